// rs_jit.hip -- the one-matrix decode through per-block generated code
// (rs_jit.h): dsts[b][i] = sum_p c_b[i][p] * srcs[b][p] with the e x k matrix
// of block b baked into code that k_jit_emit wrote into executable
// device memory (rsgpu_capi.cpp allocates it from the GPU's coarse-grained
// pool with HSA_AMD_MEMORY_POOL_EXECUTABLE_FLAG).
//
// Work split as k_rs_tc (rs_tc.hip): a workgroup of NW waves covers one 2 KB
// column tile (64 lanes x 32 bytes) of every row of one block; wave w owns
// output rows [8w, 8w+8); the waves share the loading (LDS-DMA) and bit
// transposing of each chunk of 8 sources through LDS.  Per chunk a wave makes
// ONE call into its generated code, which reads the planes from LDS, builds
// the four-Russians tables and applies its 8 x 8 coefficients: no
// per-coefficient jumps, no scalar loads of handler addresses, no GPR index
// mode.
//
// The instruction cache is not invalidated between kernel launches
// (tools/ubench_jit.hip: code rewritten between two launches runs stale
// without it), and the code of a block is rewritten by every prepare, so
// wave 0 of every workgroup executes s_icache_inv before the workgroup's
// first call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <utility>

#include "bitslice.h"
#include "diag_clock.h"
#include "plane_mul.h"
#include "rs_jit.h"
#include "rs_kernels.h"
#include "rs_lane.h"
#include "rs_pairs.h"
#include "rs_span.h"
#include "tc_handlers.inc"

namespace rsgpu {
namespace jitk {

using bs::barrier_lds;
using bs::glds32;
using bs::glds32_nt;
using bs::sload_ptr;
using bs::store32;
using bs::tr8;
using bs::vconst;
using bs::wait_vm;

constexpr int C = 8;  // sources per LDS chunk (double-buffered)

RSGPU_DIAG_TABLE

// k_rs_jitw's phase stamps (the diagnostic build's variant 6, kernel_hooks.h)
#ifdef RSGPU_DIAG_CLOCK
using JitwPhases = std::conditional_t<Hooks::kPhaseStamps, diag::PhaseTimer, diag::NoPhases>;
#else
using JitwPhases = diag::NoPhases;
#endif

// Instrumentation points of k_rs_jit.  The product instantiates JitHooks:
// no timers, every wave runs its own block's code, wave 0 invalidates the
// instruction cache.  tools/jit_profile.hip supplies its own policy (per-phase
// s_memtime sums, timing-only code substitution) without touching this file.
struct JitHooks {
    struct Timer {
        __device__ void mark(int) {}
        __device__ void end(int) {}
    };
    static constexpr bool kInvalidate = true;
    // this wave's generated code: chunk ch at code + ch * chunk_stride
    __device__ static const uint8_t* code(const JitArgs& a, bool shared, int b, int wave, int nch)
    {
        return a.code + (shared ? 0 : (size_t)b * a.block_stride) + (size_t)wave * nch * a.chunk_stride;
    }
};

template <int S>
__device__ __forceinline__ void read_slot(uint32_t (&W)[8])
{
    uint64_t P[4];
#define RSGPU_JIT_RD(TEXT) asm volatile(TEXT : "=v"(P[0]), "=v"(P[1]), "=v"(P[2]), "=v"(P[3]))
    if constexpr (S == 0) RSGPU_JIT_RD(RSGPU_TC_READ_SLOT64_0);
    if constexpr (S == 1) RSGPU_JIT_RD(RSGPU_TC_READ_SLOT64_1);
    if constexpr (S == 2) RSGPU_JIT_RD(RSGPU_TC_READ_SLOT64_2);
    if constexpr (S == 3) RSGPU_JIT_RD(RSGPU_TC_READ_SLOT64_3);
    if constexpr (S == 4) RSGPU_JIT_RD(RSGPU_TC_READ_SLOT64_4);
    if constexpr (S == 5) RSGPU_JIT_RD(RSGPU_TC_READ_SLOT64_5);
    if constexpr (S == 6) RSGPU_JIT_RD(RSGPU_TC_READ_SLOT64_6);
    if constexpr (S == 7) RSGPU_JIT_RD(RSGPU_TC_READ_SLOT64_7);
#undef RSGPU_JIT_RD
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        W[2 * q] = (uint32_t)P[q];
        W[2 * q + 1] = (uint32_t)(P[q] >> 32);
    }
}

// k_rs_jit's eight slots, as the scrub epilogue reads them
struct Slots8 {
    static constexpr int N = 8;
    template <int S>
    __device__ __forceinline__ static void read(uint32_t (&W)[8])
    {
        read_slot<S>(W);
    }
    // P ^= the slot's planes, the slot never copied out
    template <int S>
    __device__ __forceinline__ static void xor_into(uint32_t (&P)[8])
    {
#define RSGPU_JIT_XS(TEXT)                                                                                       \
    asm volatile(TEXT : "+v"(P[0]), "+v"(P[1]), "+v"(P[2]), "+v"(P[3]), "+v"(P[4]), "+v"(P[5]), "+v"(P[6]), \
                 "+v"(P[7]))
        if constexpr (S == 0) RSGPU_JIT_XS(RSGPU_TC_XOR_SLOT_0);
        if constexpr (S == 1) RSGPU_JIT_XS(RSGPU_TC_XOR_SLOT_1);
        if constexpr (S == 2) RSGPU_JIT_XS(RSGPU_TC_XOR_SLOT_2);
        if constexpr (S == 3) RSGPU_JIT_XS(RSGPU_TC_XOR_SLOT_3);
        if constexpr (S == 4) RSGPU_JIT_XS(RSGPU_TC_XOR_SLOT_4);
        if constexpr (S == 5) RSGPU_JIT_XS(RSGPU_TC_XOR_SLOT_5);
        if constexpr (S == 6) RSGPU_JIT_XS(RSGPU_TC_XOR_SLOT_6);
        if constexpr (S == 7) RSGPU_JIT_XS(RSGPU_TC_XOR_SLOT_7);
#undef RSGPU_JIT_XS
    }
};

// log / antilog tables of the scrub's cold path
alignas(16) __device__ const GfTables kGfJit = make_gf_tables();

// ---------------------------------------------------------------------------
// The scrub epilogue of the generated kernels (rsgpu_scrub_blocks under
// RSGPU_SCRUB_GENERATED; k_rs_jit_scrub, k_rs_jitw_scrub), in place of the
// parity store: scrub_tile (rs_bitsliced.hip) for a matrix known at run time.
// The wave holds rows [r0, r0 + nrow) of the computed parity as planes in its
// slots (SL: Slots8, SlotsW); dsts names the block's STORED parity rows, which
// are only read (the repair, JitRepair below, writes through bases of its own).
// Wave `wave` of NV of tile `tw` of the workgroup's TPW.
//
// Per row: the lane's 32 stored bytes (one row's load in flight ahead, no
// further), one tr8 on them -- the stored side: the slot's planes are then
// XORed in straight from the accumulators, never copied out -- and the OR of
// the syndrome planes over planes and rows
// is the lane's bad-byte mask (bit 8 q + w: byte 4 w + q).  A lane past the
// row end, and every lane of a tile past the last one, reads the row head
// (po = 0) and gives no mask (inb false); it takes every barrier below.
//
// Then a workgroup barrier (other waves may still be reading the last chunk's
// planes), and the masks meet in the chunk buffers, now free: [NV TPW][64]
// u32 at ldsb.  A clean workgroup ends there and has written nothing.  Wave 0
// of a bad tile adds the tile's bad columns to the block's fold, one 64-bit
// atomicAdd.  With `locate` the whole workgroup (the barriers are its own)
// enters the cold path, small code and not fast code: in 8 passes the waves
// lay 4 bytes per lane of all e syndrome rows into LDS (syn [e][256] per
// tile, behind the masks: kScrubMaskBytes + TPW e 256 bytes, e <= 64), and a
// tile's threads walk the 256 columns with the rule of a general locatable
// matrix (rs_lane.h scrub_locate_row; rowtab and the matrix at s.tab).  The
// maxima of row + 1 and of kScrubBias - row go into the fold, one atomicMax
// pair per wave.
// ---------------------------------------------------------------------------
constexpr int kScrubMaskBytes = 2048;  // >= 4 NV TPW 64: at most 6 waves

struct JitScrub {
    static constexpr bool kSpan = false;  // the cold path names one row per column
    static constexpr bool kRepair = false;  // scrub_slots only reads the rows
    ScrubFold* fold;
    const uint8_t* tab;
    int locate;
};

// The locate of several rows (rsgpu_locate_blocks under FUSED + GENERATED;
// k_rs_jit_locate, k_rs_jitw_locate): the same epilogue with the cold path of
// span_tile (rs_bitsliced.hip) for a matrix known at run time.  The eight
// passes lay the syndromes into LDS as above, at a row stride of kLocRow = 260
// bytes: lane p of a wave reads syndrome p of one column, byte p kLocRow + c.
// A byte or dword read is served in two groups of 32 lanes over 32 banks of 4
// bytes; at 256 bytes = 64 dwords every lane of a group would meet the same
// bank, a 32-way conflict.  260 = 65 dwords puts lane p on bank (p + c / 4)
// mod 32, every lane of a group on its own, and keeps the passes' dword writes
// (consecutive dwords of a row, no conflict either) aligned.  After a pass's
// barrier the NV waves of a tile divide the tile lanes that have a bad byte in
// it (`tm`, the tile's masks: bit 8 q + w is byte 4 w + q, so pass p owns bits
// 8 q + p and column 4 lane + q of the pass); each wave visits its columns one after the other, all
// 64 lanes on each, under wave-uniform control, and reduces them against its
// own basis of at most u vectors (rs_span.h).  After the last pass's barrier
// wave 0 of the workgroup merges the NV TPW bases -- every tile the workgroup
// owns; an idle tile past the row end has an empty one -- and writes them to
// the next free slot of the block's candidate area, claimed with an atomicAdd
// on the fold's hi1, which the locate uses for nothing else.  A block has a
// slot per 2048-byte tile and a workgroup covers at least one tile, so the
// claim is always below `slots`.  The order of the claims is that of the
// workgroups' arrival; W, the span of all the block's syndrome columns, does
// not depend on the order in which its vectors are met, and k_locate_finish
// derives every byte of its output from W and the count.
// LDS, in the chunk buffers: masks 2 KiB | syn [TPW][N NV][260] | GF tables
// 768 B | NV TPW bases of 552 B (LocLds; N NV: the most rows the layout takes).
struct JitLocate {
    static constexpr bool kSpan = true;  // the cold path keeps the span of the columns
    static constexpr bool kRepair = false;
    static constexpr int locate = 1;
    ScrubFold* fold;  // hi1 counts the block's claimed slots
    uint8_t* cand;
    size_t cand_stride;
    int slots, u;
};

// The repair (rsgpu_repair_blocks under RSGPU_REPAIR_KERNEL_GENERATED;
// k_rs_jit_repair, k_rs_jitw_repair): JitScrub's epilogue with the cold path
// correcting in its walk, as scrub_tile (rs_bitsliced.hip) does for the
// compiled codes.  The thread at column c of pass `pass` of tile `tw` has the
// row, and c is byte 4 pass + c % 4 of lane c / 4's 32 bytes of the tile, so
// the column is byte tile0 + (c >> 2) 32 + 4 pass + (c & 3) of the row: it
// XORs x = s_0 / c[0][r] into source row r (x from the tables at `tab`, the
// quotient scrub_locate_row tests the other syndromes against), or s_p0 into
// parity row k + p0.  One byte read and written per bad column, in the cold
// path only; the address comes from base, pitch and row by selects (no load
// from the row-pointer table, whose divergent 64-bit address the wide kernels
// have no registers for), and the write is one divergent region: address and
// value by selects, one `if` around the store, the fold by selects.
// In place is safe: every wave of the workgroup has read all its sources
// before the body's last barrier; a pass of the cold path reloads, per lane and
// row, only the stored-parity dword that pass owns (bytes 4 pass .. 4 pass + 3
// of the lane's 32), and a correction touches bytes of that dword alone, after
// the pass's barrier, when every wave has laid its syndromes into LDS; tiles
// are disjoint column ranges, so no other workgroup uses those bytes -- the
// idle lanes of a row's tail tile do re-read the row head, which the head's
// workgroup may be correcting, but what they read is discarded (`inb`).  An
// idle lane's syndromes are zeros, so none of its columns is bad; the column is
// checked against len all the same before a write.
// The modes are rs_kernels.h's: kRepairLocate folds every bad column and writes
// no row byte; kRepairColumns corrects, folds `row` over the corrected columns
// only and counts them in rep, one atomic per wave; kRepairGated (after the
// finalise; the kernel has left already where the block is not to be written)
// corrects and touches no field of the report.
struct JitRepair {
    static constexpr bool kSpan = false;
    static constexpr bool kRepair = true;  // scrub_slots corrects what it locates
    static constexpr int locate = 1;
    RepairFold* fold;  // [B]: zeroed (kRepairLocate, kRepairColumns) or the final reports (kRepairGated)
    const uint8_t* tab;
    int mode;
    uint8_t* src;  // [B][k] rows of the slice
    uint8_t* par;  // [B][e] rows of the slice, the stored parity
    long long pitch, len;
};

constexpr int kLocRow = 260;
template <int N, int NV, int TPW>
struct LocLds {
    static constexpr int kGfAt = kScrubMaskBytes + TPW * N * NV * kLocRow;
    static constexpr int kBasesAt = kGfAt + (int)sizeof(GfTables);
    static constexpr int kBytes = kBasesAt + NV * TPW * (int)sizeof(SpanBasis);
    static_assert(kLocRow % 4 == 0 && kGfAt % 8 == 0 && sizeof(GfTables) % 8 == 0, "dword writes, aligned bases");
    static_assert(NV == 1 || NV == 2 || NV == 4, "the waves divide the tile's 64 lanes");
};

// The correction per column (rsgpu_correct_blocks under FUSED with the scrub
// kernel GENERATED; k_rs_jit_correct, k_rs_jitw_correct): JitRepair in its
// kRepairColumns mode on the 32-byte fold.  With t == 2 a bad column that no
// row explains is pending instead of left: when a trip of the walk ends --
// thread wave 64 + lane of a tile's NV 64 takes columns wave 64 + lane, + 64 NV,
// ... of the pass's 256, so wave w owns tile lanes 16 w .. 16 w + 15 (mod 16
// NV) and makes 4 / NV trips -- the wave takes the trip's pending columns one
// at a time, all 64 lanes on each, under wave-uniform control
// (correct_pending, below), while the pass's syndromes are still in LDS,
// before the pass's closing barrier.  A two-row correction adds to `rep` and
// `two` and sets the fold's hi1 / lo1 to kScrubNoRow.  In place for
// JitRepair's reasons: the two bytes are bytes of the dword the pass owns, in
// rows whose sources every wave has read before the body's last barrier.
// LDS, in the chunk buffers (CorLds): masks | syn [TPW][e][256] | PairGf, the
// workgroup's | rows 0 to 2 of the matrix as logarithms, the workgroup's, in
// the mask part's free end where the masks leave 768 bytes | per wave
// CorRow [k].  syn keeps JitRepair's row stride of 256 bytes and not kLocRow:
// no read of this search is strided by the lane -- a column's syndromes are
// read at the same address in every lane (pair_search_lane) -- and 4 bytes
// more per row would cost the four-wave 16-row layout 8 more rows of k.
struct JitCorrect {
    static constexpr bool kSpan = false;
    static constexpr bool kRepair = true;
    static constexpr int locate = 1;
    static constexpr int mode = kRepairColumns;
    CorrectFold* fold;  // [B], zeroed
    const uint8_t* tab;
    int t;
    uint8_t* src;  // [B][k] rows of the slice
    uint8_t* par;  // [B][e] rows of the slice, the stored parity
    long long pitch, len;
    long long tile0 = 0;  // k_rs_jitw_correct: the first column of the wave's tile (JitwEpi)
};

template <int NV, int TPW>
struct CorLds {
    static constexpr int kWaves = NV * TPW;
    static constexpr int kGfBytes = ((int)sizeof(PairGf) + 7) / 8 * 8;
    static constexpr int kLogBytes = 3 * 256;
    // the masks take 4 kWaves 64 bytes of their part
    static constexpr bool kLogInMasks = 4 * kWaves * 64 + kLogBytes <= kScrubMaskBytes;
    static constexpr int gf_at(int e) { return kScrubMaskBytes + TPW * e * 256; }
    static constexpr int log_at(int e) { return kLogInMasks ? kScrubMaskBytes - kLogBytes : gf_at(e) + kGfBytes; }
    static constexpr int rows_at(int e) { return gf_at(e) + kGfBytes + (kLogInMasks ? 0 : kLogBytes); }
    static constexpr int bytes(int k, int e) { return rows_at(e) + kWaves * k * (int)sizeof(CorRow); }
    // every (k, e) of e0 <= e <= e1 with k + e <= 250
    static constexpr bool fits_all(int e0, int e1, int cap)
    {
        for (int e = e0; e <= e1; ++e)
            if (bytes(250 - e, e) > cap)
                return false;
        return true;
    }
    static_assert(sizeof(PairGf) == 1284 && sizeof(CorRow) == 8 && kScrubMaskBytes % 8 == 0 && kGfBytes % 8 == 0 &&
                      kLogBytes % 8 == 0,
                  "the rows' tables are aligned");
};

typedef __attribute__((address_space(3))) uint8_t cor_lds_u8;
typedef __attribute__((address_space(3))) const PairGf cor_lds_gf;
typedef __attribute__((address_space(3))) CorRow cor_lds_row;

// The workgroup's tables of the search, on entry to the cold path: read from
// the first pass's barrier on; the chunk buffers are free since the barrier
// before the masks.
template <int NV, int TPW>
__device__ __forceinline__ void correct_tables(const uint8_t* tab, int k, int e, uint8_t* ldsb, int tid)
{
    using Lay = CorLds<NV, TPW>;
    cor_lds_u8* gfb = (cor_lds_u8*)ldsb + Lay::gf_at(e);
    cor_lds_u8* lg = (cor_lds_u8*)ldsb + Lay::log_at(e);
#pragma unroll 1
    for (int i = tid; i < (int)sizeof(PairGf); i += 64 * NV * TPW)
        gfb[i] = pair_gf_byte(kGfJit, i);
#pragma unroll 1
    for (int r = tid; r < k; r += 64 * NV * TPW) {
        lg[r] = pair_log8(kGfJit, tab[256 + r]);
        lg[256 + r] = pair_log8(kGfJit, tab[256 + k + r]);
        lg[512 + r] = pair_log8(kGfJit, tab[256 + 2 * k + r]);
    }
}

// The pending columns of a trip of the walk (`pend`, a lane each; lane 0's is
// column c0 of the pass), one after the other, the whole wave on each: the
// search of rs_correct.hip's head on the tables above, the lanes' matches
// counted up to two, and the lane that holds the only one XORs both bytes into
// the global rows; two matching pairs, or none, leave the column byte for
// byte.  Returns the columns corrected, the same in every lane.
template <int NV, int TPW>
__device__ __forceinline__ unsigned correct_pending(const JitCorrect& s, bool pend, int c0, int pass, int k, int e,
                                                    int b, long long tile0, int lane, int slot, int tw,
                                                    uint8_t* ldsb)
{
    using Lay = CorLds<NV, TPW>;
    unsigned long long todo = __ballot(pend);
    if (!todo)
        return 0;
    cor_lds_u8* syn = (cor_lds_u8*)ldsb + kScrubMaskBytes + tw * e * 256;
    cor_lds_gf* gf = (cor_lds_gf*)((cor_lds_u8*)ldsb + Lay::gf_at(e));
    cor_lds_u8* lg = (cor_lds_u8*)ldsb + Lay::log_at(e);
    cor_lds_row* row = (cor_lds_row*)((cor_lds_u8*)ldsb + Lay::rows_at(e)) + slot * k;
    unsigned done = 0;
    while (todo) {
        const int c = c0 + __ffsll(todo) - 1;
        todo &= todo - 1;
        // what every lane reads at one address goes to a scalar register
        auto uniform = [](unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); };
        const unsigned ls0 = uniform(pair_logp(gf, syn[c])), ls1 = uniform(pair_logp(gf, syn[256 + c])),
                       ls2 = uniform(pair_logp(gf, syn[512 + c]));
#pragma unroll 1
        for (int r = lane; r < k; r += 64) {
            const CorRow v = pair_row(gf, ls0, ls1, ls2, lg[r], lg[256 + r], lg[512 + r]);
            row[r].a0 = v.a0;
            row[r].a1 = v.a1;
            row[r].c2 = v.c2;
            row[r].u = v.u;
        }
        // what a lane wrote is read by the other lanes of the wave from here on
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const CorPairs p = pair_hits(pair_search_lane(gf, k, e, syn + c, 256, lg, lg + 256, lg + 512, row,
                                                      (const g_u8*)(s.tab + 256), lane, uniform));
        const long long col = tile0 + (c >> 2) * 32 + 4 * pass + (c & 3);
        const bool one = __ballot(p.cnt >= 2) == 0 && __popcll(__ballot(p.cnt == 1)) == 1 && col < s.len;
        if (one && p.cnt == 1) {
            g_u8* ga = (g_u8*)(p.ra < k ? s.src + ((size_t)b * k + p.ra) * s.pitch
                                        : s.par + ((size_t)b * e + (p.ra - k)) * s.pitch) + col;
            g_u8* gb = (g_u8*)(p.rb < k ? s.src + ((size_t)b * k + p.rb) * s.pitch
                                        : s.par + ((size_t)b * e + (p.rb - k)) * s.pitch) + col;
            *ga ^= p.xa;
            *gb ^= p.xb;
        }
        done += one;
        // the next column's rows overwrite what the lanes still read here
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    return done;
}

template <class SL, int NV, int TPW, class S>
__device__ __forceinline__ void scrub_slots(const S& s, int k, int e, uint8_t* const* dsts, int b, int r0,
                                            int nrow, int wave, int tw, bool inb, uint32_t po, uint8_t* ldsb,
                                            uint32_t m4, uint32_t m2, uint32_t m1,
                                            [[maybe_unused]] long long tile0 = 0)  // the repair: the tile's first column
{
    static_assert(4 * NV * TPW * 64 <= kScrubMaskBytes, "the masks fit their part");
    // the lane index afresh: the body's copy, kept live to the end of the cold
    // path, cost k_rs_jitw_scrub one VGPR spilled to scratch across its main
    // loop (9 registers survive the call there)
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    // the stored rows' pointers: scalar loads under one wait, clamped in bounds
    typedef const uint8_t* const __attribute__((address_space(4)))* CRows;
    const uint8_t* dp[SL::N];
#pragma unroll
    for (int i = 0; i < SL::N; ++i)
        dp[i] = ((CRows)dsts)[min(r0 + i, e - 1)];
    uint32_t mine = 0;
    uint32_t Pn[8];
    bs::load32(dp[0], po, true, Pn);
    [&]<int... Ss>(std::integer_sequence<int, Ss...>) {
        (
            [&] {
                if (Ss < nrow) {
                    uint32_t Pw[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        Pw[q] = Pn[q];
                    if constexpr (Ss + 1 < SL::N)
                        if (Ss + 1 < nrow)
                            bs::load32(dp[Ss + 1], po, true, Pn);
                    tr8(Pw, m4, m2, m1);
                    SL::template xor_into<Ss>(Pw);  // the syndromes, as planes
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        mine |= Pw[q];
                    __builtin_amdgcn_sched_barrier(0);
                }
            }(),
            ...);
    }(std::make_integer_sequence<int, SL::N>{});
    uint32_t* wmask = reinterpret_cast<uint32_t*>(ldsb);
    __syncthreads();
    wmask[(tw * NV + wave) * 64 + lane] = inb ? mine : 0u;
    __syncthreads();
    uint32_t tm = 0, any = 0;  // this lane's columns: of the tile, of the workgroup
#pragma unroll
    for (int g = 0; g < NV * TPW; ++g) {
        const uint32_t m = wmask[g * 64 + lane];
        any |= m;
        tm |= g / NV == tw ? m : 0u;
    }
    if (__ballot(any != 0) == 0)
        return;  // the same for every wave of the workgroup
    auto* f = s.fold + b;
    if (wave == 0) {
        unsigned n = __builtin_popcount(tm);
        for (int o = 32; o > 0; o >>= 1)
            n += __shfl_down(n, o, 64);
        bool count = lane == 0 && n;
        if constexpr (S::kRepair)
            count = count && s.mode != kRepairGated;  // the block's report is final
        if (count)
            atomicAdd(&f->bad, (unsigned long long)n);
    }
    if (!s.locate)
        return;
    // LDS through its own address space, the stored dword through an SGPR base
    // and one VGPR offset, every loop rolled: what the compiler would otherwise
    // hoist out of the pass loop (a 64-bit address per slot and row) took
    // k_rs_jitw_scrub's allocation past v39, into the accumulators -- num_vgpr
    // is no hard limit below 64 registers
    typedef __attribute__((address_space(3))) uint8_t lds_u8;
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    constexpr int kRow = S::kSpan ? kLocRow : 256;
    lds_u8* syn = (lds_u8*)ldsb + kScrubMaskBytes + tw * e * kRow;
    [[maybe_unused]] unsigned hi1 = 0, lo1 = 0, nrep = 0;
    using Lay = LocLds<SL::N, NV, TPW>;
    [[maybe_unused]] GfTables& gf = *reinterpret_cast<GfTables*>(ldsb + Lay::kGfAt);
    [[maybe_unused]] SpanBasis* sb = reinterpret_cast<SpanBasis*>(ldsb + Lay::kBasesAt);
    if constexpr (S::kSpan) {
        // read from the first pass's barrier on; the chunk buffers are free
        // since the barrier before the masks
        load_gf_rolled(gf, kGfJit, (tw * NV + wave) * 64 + lane, 64 * NV * TPW);
        sb[tw * NV + wave].n = 0;
        sb[tw * NV + wave].ovf = 0;
    }
    constexpr bool kCorrect = std::is_same_v<S, JitCorrect>;
    [[maybe_unused]] unsigned ntwo = 0;  // the correction: the wave's columns corrected in two rows
    if constexpr (kCorrect)
        if (s.t == 2)
            correct_tables<NV, TPW>(s.tab, k, e, ldsb, (tw * NV + wave) * 64 + lane);
#pragma unroll 1
    for (int pass = 0; pass < 8; ++pass) {
        // bytes 4 pass .. 4 pass + 3 of the lane's 32 of every row (zeros from an idle lane)
        lds_u32* mine4 = (lds_u32*)(syn + r0 * kRow + lane * 4);
        const uint32_t po4 = po + 4 * pass;
        // the correction: the transposes' masks afresh per pass, so that they
        // are not live across the pair search of the pass before
        uint32_t p4 = m4, p2 = m2, p1 = m1;
        if constexpr (kCorrect) {
            p4 = vconst(0x0F0F0F0Fu);
            p2 = vconst(0x33333333u);
            p1 = vconst(0x55555555u);
        }
        [&]<int... Ss>(std::integer_sequence<int, Ss...>) {
            (
                [&] {
                    if (Ss < nrow) {
                        uint32_t W[8], st;
                        // (s_nop 4: the row pointer may come straight from a
                        // v_readlane -- k_rs_jitw_scrub<J16> keeps some of its 16 in
                        // VGPR lanes -- and a VALU write of an SGPR needs 5 wait
                        // states before a vector memory instruction reads it; the
                        // compiler does not look into asm text for that)
                        asm volatile("s_nop 4\n global_load_dword %0, %1, %2\n s_waitcnt vmcnt(0)"
                                     : "=v"(st)
                                     : "v"(po4), "s"(dp[Ss])
                                     : "memory");
                        SL::template read<Ss>(W);
                        tr8(W, p4, p2, p1);  // computed parity, bytes
                        uint32_t d = W[0];
#pragma unroll
                        for (int q = 1; q < 8; ++q)
                            d = pass == q ? W[q] : d;
                        mine4[Ss * (kRow / 4)] = inb ? d ^ st : 0u;
                        __builtin_amdgcn_sched_barrier(0);  // slot by slot
                    }
                }(),
                ...);
        }(std::make_integer_sequence<int, SL::N>{});
        __syncthreads();
        if constexpr (S::kSpan) {
            // tile lanes wave, wave + NV, ... are this wave's
            constexpr unsigned long long kShare =
                NV == 1 ? ~0ull : NV == 2 ? 0x5555555555555555ull : 0x1111111111111111ull;
            SpanBasis& mb = sb[tw * NV + wave];
            unsigned pm = 0;  // bit q: column 4 lane + q of the pass is bad
#pragma unroll
            for (int q = 0; q < 4; ++q)
                pm |= ((tm >> (8 * q + pass)) & 1u) << q;
            unsigned long long todo = __ballot(pm != 0) & (kShare << wave);
            while (todo) {
                const int from = __ffsll(todo) - 1;
                todo &= todo - 1;
                unsigned m = (unsigned)__builtin_amdgcn_readlane((int)pm, from);
                while (m) {
                    const int c = from * 4 + __ffs(m) - 1;
                    m &= m - 1;
                    const uint8_t v = lane < e ? syn[lane * kRow + c] : (uint8_t)0;
                    span_append(mb, gf, lane, span_reduce(mb, gf, lane, v), s.u);
                }
            }
        } else {
            // The correction: a trip's pending column (bad, no row explains it)
            // goes to the wave when the trip ends, by `continue` or not: the
            // trip count is the same in every lane, all 64 are there.
            [[maybe_unused]] bool pend = false;
            auto trip_ends = [&]([[maybe_unused]] int c) {
                if constexpr (kCorrect) {
                    if (s.t == 2)
                        ntwo += correct_pending<NV, TPW>(s, pend, __builtin_amdgcn_readfirstlane(c - lane), pass, k, e,
                                                         b, tile0, lane, tw * NV + wave, tw, ldsb);
                    pend = false;
                }
            };
            for (int c = wave * 64 + lane; c < 256; trip_ends(c), c += 64 * NV) {
                int nz = 0, p0 = 0;
#pragma unroll 1
                for (int p = 0; p < e; ++p) {
                    const bool on = syn[p * 256 + c] != 0;
                    nz += on;
                    p0 = on ? p : p0;
                }
                if (!nz)
                    continue;
                // locate: the matrix is locatable, so e >= 2
                const int row = scrub_locate_row(k, e, s.tab, s.tab + 256, kGfJit, syn[c], syn[256 + c], nz, p0,
                                                 [&](int p) { return syn[p * 256 + c]; });
                if constexpr (S::kRepair) {
                    const bool src_row = row < k;
                    const long long col = tile0 + (c >> 2) * 32 + 4 * pass + (c & 3);
                    g_u8* g = (g_u8*)(src_row ? s.src : s.par) +
                              ((size_t)b * (src_row ? k : e) + (src_row ? row : row - k)) * s.pitch + col;
                    // x = s_0 / c[0][r] (c[0][r] != 0: the matrix is locatable), or s_p0
                    const int ls = kGfJit.log[syn[c]] + 255 - kGfJit.log[s.tab[256 + (row >= 0 && src_row ? row : 0)]];
                    const uint8_t x = src_row ? kGfJit.exp[ls] : syn[(src_row ? 0 : row - k) * 256 + c];
                    if (s.mode != kRepairLocate && row >= 0 && col < s.len) {
                        *g ^= x;
                        ++nrep;
                    }
                    // what folds into `row`: every bad column (kRepairLocate), the
                    // corrected ones (kRepairColumns), none (kRepairGated)
                    const bool folds = s.mode == kRepairLocate || (s.mode == kRepairColumns && row >= 0);
                    hi1 = max(hi1, !folds ? 0u : row >= 0 ? (unsigned)row + 1 : kScrubNoRow);
                    lo1 = max(lo1, !folds ? 0u : row >= 0 ? kScrubBias - (unsigned)row : kScrubNoRow);
                    if constexpr (kCorrect)
                        pend = row < 0;
                    continue;
                }
                hi1 = max(hi1, row >= 0 ? (unsigned)row + 1 : kScrubNoRow);
                lo1 = max(lo1, row >= 0 ? kScrubBias - (unsigned)row : kScrubNoRow);
            }
        }
        __syncthreads();  // the next pass overwrites syn; the last one: the bases are complete
    }
    if constexpr (S::kSpan) {
        // one slot per dirty workgroup; any order of the claims gives the same
        // span W of the block, and so the same output (above)
        if (tw * NV + wave == 0) {
            unsigned at = 0;
            if (lane == 0)
                at = atomicAdd(&f->hi1, 1u);
            at = (unsigned)uni((int)at);
            if (at < (unsigned)s.slots)  // always, with hi1 zero before the launch
                span_publish_rolled(sb[0], sb, NV * TPW, gf, lane, s.u,
                                    s.cand + (size_t)b * s.cand_stride + (size_t)at * kLocateSlotBytes);
        }
        return;
    }
    if constexpr (kCorrect) {
        // a two-row correction: no common row of the block's corrected columns
        hi1 = ntwo ? kScrubNoRow : hi1;
        lo1 = ntwo ? kScrubNoRow : lo1;
        nrep += lane == 0 ? ntwo : 0u;
        if (lane == 0 && ntwo)
            atomicAdd(&f->two, (unsigned long long)ntwo);
    }
    for (int o = 32; o > 0; o >>= 1) {
        hi1 = max(hi1, (unsigned)__shfl_down((int)hi1, o, 64));
        lo1 = max(lo1, (unsigned)__shfl_down((int)lo1, o, 64));
    }
    if (lane == 0 && hi1) {
        atomicMax(&f->hi1, hi1);
        atomicMax(&f->lo1, lo1);
    }
    if constexpr (S::kRepair) {
        for (int o = 32; o > 0; o >>= 1)
            nrep += __shfl_down(nrep, o, 64);
        if (lane == 0 && nrep && s.mode == kRepairColumns)
            atomicAdd(&f->rep, (unsigned long long)nrep);
    }
}

// The first column of the tile whose lanes sit at `off` (lane 0: the tile's
// start), as a scalar, for the repair's cold path.  (From `off` and not from
// the 32-bit offset the loads use, lane 0's where it is live: that form cost
// k_rs_jitw_repair<J16> a VGPR pair spilled to scratch, and clean (14, 32)
// blocks 6 % against the scrub; profiles/repair_generated/.)
__device__ __forceinline__ long long tile_start(long long off)
{
    return (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(off >> 32)) << 32) |
                       (unsigned)__builtin_amdgcn_readfirstlane((int)off));
}

// The epilogues of k_rs_jit's body (jit_run).  The store: outputs back to
// bytes and out (every source of this tile was read before the last barrier).
struct JitStore {
    template <int NW>
    __device__ __forceinline__ void run(const JitArgs& a, uint8_t* const* const& dsts, int, const int& wave, int,
                                        const long long& off, uint4*, const uint32_t& m4, const uint32_t& m2,
                                        const uint32_t& m1) const
    {
        if (off + 32 <= a.len) {
            [&]<int... Ss>(std::integer_sequence<int, Ss...>) {
                (
                    [&] {
                        const int r = wave * 8 + Ss;
                        if (r < a.rows) {
                            uint32_t W[8];
                            read_slot<Ss>(W);
                            tr8(W, m4, m2, m1);
                            store32((uint8_t*)sload_ptr((const uint8_t* const*)(dsts + r)), off, W);
                        }
                    }(),
                    ...);
            }(std::make_integer_sequence<int, 8>{});
        }
    }
};

// The scrub (S = JitScrub) and the locate (JitLocate): wave w's rows [8 w, 8 w
// + 8) against the stored ones
template <class S>
struct JitEpi8 : S {
    template <int NW>
    __device__ __forceinline__ void run(const JitArgs& a, uint8_t* const* dsts, int b, int wave, int,
                                        long long off, uint4* lds, uint32_t m4, uint32_t m2, uint32_t m1) const
    {
        static_assert(kScrubMaskBytes + 32 * 256 <= 2 * C * 2 * 64 * 16, "rows <= 32: syn fits the chunk buffers");
        static_assert(!S::kSpan || LocLds<8, NW, 1>::kBytes <= 2 * C * 2 * 64 * 16,
                      "rows <= 8 NW: masks, syn, tables and bases fit the chunk buffers");
        static_assert(!std::is_same_v<S, JitCorrect> || CorLds<NW, 1>::fits_all(1, 8 * NW, 2 * C * 2 * 64 * 16),
                      "rows <= 8 NW: the correction's tables fit the chunk buffers at every k");
        const bool inb = off + 32 <= a.len;
        if constexpr (S::kRepair)
            scrub_slots<Slots8, NW, 1>(static_cast<const S&>(*this), a.k, a.rows, dsts, b, wave * 8,
                                       min(8, a.rows - wave * 8), wave, 0, inb, inb ? (uint32_t)off : 0u,
                                       reinterpret_cast<uint8_t*>(lds), m4, m2, m1, tile_start(off));
        else
            scrub_slots<Slots8, NW, 1>(static_cast<const S&>(*this), a.k, a.rows, dsts, b, wave * 8,
                                       min(8, a.rows - wave * 8), wave, 0, inb, inb ? (uint32_t)off : 0u,
                                       reinterpret_cast<uint8_t*>(lds), m4, m2, m1);
    }
};
using JitScrub8 = JitEpi8<JitScrub>;
using JitLocate8 = JitEpi8<JitLocate>;
using JitRepair8 = JitEpi8<JitRepair>;
using JitCorrect8 = JitEpi8<JitCorrect>;

// `int B` and `long long TILE`: this workgroup's block and its tile
// (k_rs_jitw: its index) within the block.  Workgroups are dealt round-robin
// over the 8 XCDs: A.xcd_order gives each XCD a contiguous range of (block,
// tile), so all tiles of a block (and its code) stay in one XCD's L2 -- it
// matters when a block has few tiles.  (A macro: as a function taking
// references it changed the code of k_rs_jit and k_rs_jitw.)
#define RSGPU_JIT_PLACE(A, B, TILE)                                                                 \
    int B = blockIdx.y;                                                                             \
    long long TILE = blockIdx.x;                                                                    \
    if ((A).xcd_order) {                                                                            \
        const unsigned g = blockIdx.x + gridDim.x * blockIdx.y, tot = gridDim.x * gridDim.y;        \
        const unsigned xcd = g & 7, q8 = tot >> 3, r8 = tot & 7;                                    \
        const unsigned lin = xcd * q8 + min(xcd, r8) + (g >> 3);                                    \
        B = (int)(lin / gridDim.x);                                                                 \
        TILE = lin - (unsigned)B * gridDim.x;                                                       \
    }

// The body of k_rs_jit and k_rs_jit_scrub on block b, tile `tile`: the
// accumulation, then the epilogue `epi` on the wave's slots (JitStore,
// JitScrub8).  The kernels place the workgroup (RSGPU_JIT_PLACE) and skip a
// block by its status themselves: a `return` in here would be a branch to the
// kernel's one exit, and k_rs_jit's code another than it was.
template <int NW, bool SH, class H, class Epi>
__device__ __forceinline__ void jit_run(const JitArgs& a, uint4 (&lds)[2][C * 2 * 64], int wave, int lane, int b,
                                        long long tile, const Epi& epi)
{
    const int k = a.k;
    const int nch = (k + C - 1) / C;
    const uint8_t* const* srcs = a.srcs + (size_t)b * k;
    uint8_t* const* dsts = a.dsts + (size_t)b * a.dst_stride;
    const uint8_t* code = H::code(a, SH, b, wave, nch);
    const uint32_t m4 = vconst(0x0F0F0F0Fu), m2 = vconst(0x33333333u), m1 = vconst(0x55555555u);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4*)&lds[0][0];
    const long long off = tile * 2048 + lane * 32;
    const long long loff = off + 32 <= a.len ? off : 0;  // out-of-range lanes re-read the row head

    // The instruction cache is shared by the waves of a CU pair and keeps
    // lines across launches: wave 0 invalidates it before any wave of this
    // workgroup calls code (the calls follow the first chunk barrier).  Every
    // wave invalidating measured 1.3 % slower (it wipes the other workgroups'
    // lines too; profiles/r02_ab/jit_icache_inv.log).
    if (H::kInvalidate && wave == 0)
        asm volatile("s_icache_inv\n s_nop 15\n s_nop 15" ::: "memory");

    // chunk ch's sources this wave moves: t = wave, wave + NW, ... (two row
    // pointers per scalar wait)
    auto issue = [&](int ch) {
        const int c0 = ch * C, nt = min(C, k - c0);
        const uint32_t base = lds0 + (uint32_t)((ch & 1) * C * 2 * 64 * 16);
        int t = wave;
        for (; t + NW < nt; t += 2 * NW) {
            const uint8_t *r0, *r1;
            asm volatile("s_load_dwordx2 %0, %2, 0\n s_load_dwordx2 %1, %3, 0\n s_waitcnt lgkmcnt(0)"
                         : "=&s"(r0), "=&s"(r1)
                         : "s"(srcs + c0 + t), "s"(srcs + c0 + t + NW)
                         : "memory");
            glds32(r0, (uint32_t)loff, base + (uint32_t)(t * 2 * 64 * 16));
            glds32(r1, (uint32_t)loff, base + (uint32_t)((t + NW) * 2 * 64 * 16));
        }
        if (t < nt)
            glds32(sload_ptr(srcs + c0 + t), (uint32_t)loff, base + (uint32_t)(t * 2 * 64 * 16));
    };

    asm volatile(RSGPU_TC_ZERO ::: RSGPU_TC_ACC_CLOBBERS);
    typename H::Timer jp;
    issue(0);
    jp.mark(3);
    for (int ch = 0; ch < nch; ++ch) {
        const int nt = min(C, k - ch * C);
        uint4* buf = lds[ch & 1];
        wait_vm(0);  // this chunk's own sources, issued behind the previous barrier
        jp.mark(0);
        if (a.prio)  // the transposes up to the barrier over other waves' code (as k_rs_jitw)
            asm volatile("s_setprio 2" ::: "memory");
        // own share of this chunk: bytes -> bit-planes, in place, two
        // sources at a time (both sets of LDS reads in flight together)
        int t = wave;
        for (; t + NW < nt; t += 2 * NW) {
            const int t1 = t + NW;
            uint4 u0 = buf[(t * 2 + 0) * 64 + lane], v0 = buf[(t * 2 + 1) * 64 + lane];
            uint4 u1 = buf[(t1 * 2 + 0) * 64 + lane], v1 = buf[(t1 * 2 + 1) * 64 + lane];
            uint32_t W0[8] = {u0.x, u0.y, u0.z, u0.w, v0.x, v0.y, v0.z, v0.w};
            uint32_t W1[8] = {u1.x, u1.y, u1.z, u1.w, v1.x, v1.y, v1.z, v1.w};
            tr8(W0, m4, m2, m1);
            tr8(W1, m4, m2, m1);
            buf[(t * 2 + 0) * 64 + lane] = make_uint4(W0[0], W0[1], W0[2], W0[3]);
            buf[(t * 2 + 1) * 64 + lane] = make_uint4(W0[4], W0[5], W0[6], W0[7]);
            buf[(t1 * 2 + 0) * 64 + lane] = make_uint4(W1[0], W1[1], W1[2], W1[3]);
            buf[(t1 * 2 + 1) * 64 + lane] = make_uint4(W1[4], W1[5], W1[6], W1[7]);
        }
        if (t < nt) {
            uint4 u = buf[(t * 2 + 0) * 64 + lane];
            uint4 v = buf[(t * 2 + 1) * 64 + lane];
            uint32_t W[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
            tr8(W, m4, m2, m1);
            buf[(t * 2 + 0) * 64 + lane] = make_uint4(W[0], W[1], W[2], W[3]);
            buf[(t * 2 + 1) * 64 + lane] = make_uint4(W[4], W[5], W[6], W[7]);
        }
        jp.mark(1);
        barrier_lds();
        if (a.prio)
            asm volatile("s_setprio 0" ::: "memory");
        jp.mark(2);
        // one barrier per chunk: every wave is past its call of chunk ch - 1,
        // which read buffer (ch + 1) & 1, so chunk ch + 1 may land there now
        if (ch + 1 < nch)
            issue(ch + 1);
        jp.mark(3);
        const uint32_t la = lds0 + (uint32_t)((ch & 1) * C * 2 * 64 * 16) + lane * 16;
        const uint8_t* fn = code + (size_t)ch * a.chunk_stride;
        asm volatile("s_swappc_b64 s[82:83], %[fn]"
                     :
                     : [fn] "s"(fn), "{v20}"(la)
                     : "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34",
                       "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45",
                       "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56",
                       "v57", "v58", "v59", "v60", "v61", "s82", "s83", "scc", "memory",
                       RSGPU_TC_ACC_CLOBBERS);
        jp.mark(4);
    }
    epi.template run<NW>(a, dsts, b, wave, lane, off, &lds[0][0], m4, m2, m1);
    jp.mark(5);
    jp.end(lane);
}

// amdgpu_num_vgpr(64): the compiler allocates v0..v63 only (minus the
// registers the call clobbers); the accumulators v64..v127 are touched by asm
// and generated code alone.  (Holding the block's row pointers in VGPRs and
// reading them with v_readlane instead of scalar loads measured slower:
// 26.3 vs 25.1 ms at C3, tools/jit_profile.)
// SH: one program shared by every block (the GENERATED encode; a distinct
// symbol, so profiles tell it from the per-block decode)
template <int NW, bool SH, class H = JitHooks>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_num_vgpr(64))) void k_rs_jit(JitArgs a)
{
    __shared__ uint4 lds[2][C * 2 * 64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    RSGPU_JIT_PLACE(a, b, tile)
    if (a.status && a.status[b] != 0)
        return;  // uniform per workgroup: the whole block is skipped
    jit_run<NW, SH, H>(a, lds, wave, lane, b, tile, JitStore{});
}

// Block b's own length for the batched entries below (rsgpu_ec_encode_data_batch):
// lo[b], which k_ec_batch_classify wrote, through the constant address space,
// a scalar load into an SGPR.
__device__ __forceinline__ int batch_lo(const int* lo, int b)
{
    return ((const int __attribute__((address_space(4)))*)lo)[b];
}
// ... and whether the workgroup whose first tile is `tile` has nothing to do:
// in 32 bits (lo[b] >= 0, and the grid covers less than 2^31 bytes plus a
// workgroup), so that the compare is a scalar one
__device__ __forceinline__ bool batch_past(long long tile, int len)
{
    return (unsigned)tile * 2048u >= (unsigned)len;
}

// k_rs_jit<NW, true> over [0, lo[b]) of block b, a length per block: the grid
// covers the host's bound of every lo[b], and a workgroup whose tile starts at
// or behind its block's lo[b] leaves before it touches a pointer or LDS (the
// test is the same for the whole workgroup, in scalar registers).  The others
// run the body on a copy of the arguments with lo[b] as the length.
template <int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_num_vgpr(64))) void k_rs_jit_batch(JitArgs a,
                                                                                               const int* lo)
{
    __shared__ uint4 lds[2][C * 2 * 64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    RSGPU_JIT_PLACE(a, b, tile)
    const int len = batch_lo(lo, b);
    if (batch_past(tile, len))
        return;
    JitArgs ab = a;
    ab.len = len;
    jit_run<NW, true, JitHooks>(ab, lds, wave, lane, b, tile, JitStore{});
}

// The generated scrub for e <= 16: k_rs_jit<NW, true>'s accumulation on the
// matrix's shared program, then the scrub epilogue (scrub_slots)
template <int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_num_vgpr(64))) void k_rs_jit_scrub(JitScrubArgs s)
{
    __shared__ uint4 lds[2][C * 2 * 64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    RSGPU_JIT_PLACE(s.j, b, tile)
    jit_run<NW, true, JitHooks>(s.j, lds, wave, lane, b, tile, JitScrub8{{s.fold, s.tab, s.locate}});
}

// The generated locate for e <= 16: k_rs_jit_scrub with the span cold path
// (JitLocate above)
template <int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_num_vgpr(64))) void k_rs_jit_locate(JitLocateArgs s)
{
    __shared__ uint4 lds[2][C * 2 * 64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    RSGPU_JIT_PLACE(s.j, b, tile)
    jit_run<NW, true, JitHooks>(s.j, lds, wave, lane, b, tile,
                                JitLocate8{{s.fold, s.cand, s.cand_stride, s.slots, s.u}});
}

// The generated repair for e <= 16: k_rs_jit_scrub with the correcting cold
// path (JitRepair above).  kRepairGated runs after the finalise of a
// kRepairLocate pass on the same stream: the block's report is final, and a
// workgroup whose block is not REPAIRED leaves before it loads anything.
template <int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_num_vgpr(64))) void k_rs_jit_repair(JitRepairArgs s)
{
    __shared__ uint4 lds[2][C * 2 * 64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    RSGPU_JIT_PLACE(s.j, b, tile)
    if (s.mode == kRepairGated && s.fold[b].hi1 != kRepairGate)
        return;  // uniform per workgroup
    jit_run<NW, true, JitHooks>(s.j, lds, wave, lane, b, tile,
                                JitRepair8{{s.fold, s.tab, s.mode, s.src, s.par, s.pitch, s.j.len}});
}

// The generated correction for e <= 16: k_rs_jit_repair in its kRepairColumns
// mode whose cold path, with t == 2, takes the columns no row explains to
// correct_pending (JitCorrect above)
template <int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_num_vgpr(64))) void k_rs_jit_correct(JitCorrectArgs s)
{
    __shared__ uint4 lds[2][C * 2 * 64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    RSGPU_JIT_PLACE(s.j, b, tile)
    jit_run<NW, true, JitHooks>(s.j, lds, wave, lane, b, tile,
                                JitCorrect8{{s.fold, s.tab, s.t, s.src, s.par, s.pitch, s.j.len}});
}

template <int S>
__device__ __forceinline__ void read_slotw(uint32_t (&W)[8])
{
    uint64_t P[4];
#define RSGPU_JW_RD(TEXT) asm volatile(TEXT : "=v"(P[0]), "=v"(P[1]), "=v"(P[2]), "=v"(P[3]))
    if constexpr (S == 0) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_0);
    if constexpr (S == 1) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_1);
    if constexpr (S == 2) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_2);
    if constexpr (S == 3) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_3);
    if constexpr (S == 4) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_4);
    if constexpr (S == 5) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_5);
    if constexpr (S == 6) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_6);
    if constexpr (S == 7) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_7);
    if constexpr (S == 8) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_8);
    if constexpr (S == 9) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_9);
    if constexpr (S == 10) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_10);
    if constexpr (S == 11) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_11);
    if constexpr (S == 12) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_12);
    if constexpr (S == 13) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_13);
    if constexpr (S == 14) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_14);
    if constexpr (S == 15) RSGPU_JW_RD(RSGPU_JW_READ_SLOT64_15);
#undef RSGPU_JW_RD
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        W[2 * q] = (uint32_t)P[q];
        W[2 * q + 1] = (uint32_t)(P[q] >> 32);
    }
}

// k_rs_jitw's R slots, as the scrub epilogue reads them
template <int R>
struct SlotsW {
    static constexpr int N = R;
    template <int S>
    __device__ __forceinline__ static void read(uint32_t (&W)[8])
    {
        read_slotw<S>(W);
    }
    template <int S>
    __device__ __forceinline__ static void xor_into(uint32_t (&P)[8])
    {
#define RSGPU_JW_XS(TEXT)                                                                                        \
    asm volatile(TEXT : "+v"(P[0]), "+v"(P[1]), "+v"(P[2]), "+v"(P[3]), "+v"(P[4]), "+v"(P[5]), "+v"(P[6]), \
                 "+v"(P[7]))
        if constexpr (S == 0) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_0);
        if constexpr (S == 1) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_1);
        if constexpr (S == 2) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_2);
        if constexpr (S == 3) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_3);
        if constexpr (S == 4) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_4);
        if constexpr (S == 5) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_5);
        if constexpr (S == 6) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_6);
        if constexpr (S == 7) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_7);
        if constexpr (S == 8) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_8);
        if constexpr (S == 9) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_9);
        if constexpr (S == 10) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_10);
        if constexpr (S == 11) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_11);
        if constexpr (S == 12) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_12);
        if constexpr (S == 13) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_13);
        if constexpr (S == 14) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_14);
        if constexpr (S == 15) RSGPU_JW_XS(RSGPU_JW_XOR_SLOT_15);
#undef RSGPU_JW_XS
    }
};

// The epilogues of k_rs_jitw's body (jitw_run): the store ...
struct JitwStore {
    template <class W, int TPW, int NV>
    __device__ __forceinline__ void run(const JitArgs& a, uint8_t* const* const& dsts, int, const int& wave, int,
                                        int, const long long& off, uint4*) const
    {
        constexpr int R = W::R;
        // the output pointers likewise: all R loads under one wait
        typedef uint8_t* const __attribute__((address_space(4)))* CDsts;
        const int r0 = jit::wide_row0(a.rows, wave), nrow = jit::wide_row0(a.rows, wave + 1) - r0;
        uint8_t* dp[R];
#pragma unroll
        for (int i = 0; i < R; ++i)
            dp[i] = ((CDsts)dsts)[min(r0 + i, a.rows - 1)];
        if (off + 32 <= a.len) {
            const uint32_t m4 = vconst(0x0F0F0F0Fu), m2 = vconst(0x33333333u), m1 = vconst(0x55555555u);
            [&]<int... Ss>(std::integer_sequence<int, Ss...>) {
                (
                    [&] {
                        if (Ss < nrow) {
                            uint32_t Wd[8];
                            read_slotw<Ss>(Wd);
                            tr8(Wd, m4, m2, m1);
                            store32(dp[Ss], off, Wd);
                        }
                    }(),
                    ...);
            }(std::make_integer_sequence<int, R>{});
        }
    }
};

// ... and the scrub: the wave's rows [wide_row0(e, wave), wide_row0(e, wave +
// 1)) against the stored ones.  (tile index >= ntile with TPW > 1: off is
// past the row end, so every lane of that tile is idle.)
template <class S>
struct JitwEpi : S {
    template <class W, int TPW, int NV>
    __device__ __forceinline__ void run(const JitArgs& a, uint8_t* const* dsts, int b, int wave, int tw, int,
                                        long long off, uint4* lds) const
    {
        static_assert(kScrubMaskBytes + TPW * (NV == 4 ? 64 : 32) * 256 <= 2 * TPW * W::CS * 2 * 64 * 16,
                      "e <= 32 (two waves), e <= 64 (four): syn fits the chunk buffers");
        static_assert(!S::kSpan || LocLds<W::R, NV, TPW>::kBytes <= 2 * TPW * W::CS * 2 * 64 * 16,
                      "e <= R NV: masks, syn, tables and bases fit the chunk buffers");
        // the correction's tables: at every k, but for the four waves of 16
        // rows, whose bound is correct_fits' (256 e + 32 k <= 21240 there)
        static_assert(!std::is_same_v<S, JitCorrect> || (NV == 4 && W::R == 16) ||
                          CorLds<NV, TPW>::fits_all(1, NV * W::R, 2 * TPW * W::CS * 2 * 64 * 16),
                      "e <= R NV: the correction's tables fit the chunk buffers at every k");
        static_assert(!std::is_same_v<S, JitCorrect> || !(NV == 4 && W::R == 16) ||
                          (CorLds<4, 1>::fits_all(1, 59, 2 * W::CS * 2 * 64 * 16) &&
                           CorLds<4, 1>::bytes(151, 64) <= 2 * W::CS * 2 * 64 * 16 &&
                           CorLds<4, 1>::bytes(152, 64) > 2 * W::CS * 2 * 64 * 16),
                      "four waves of 16 rows: every k up to e = 59, k <= 151 at e = 64");
        const uint32_t m4 = vconst(0x0F0F0F0Fu), m2 = vconst(0x33333333u), m1 = vconst(0x55555555u);
        const int r0 = jit::wide_row0(a.rows, wave), nrow = jit::wide_row0(a.rows, wave + 1) - r0;
        if constexpr (std::is_same_v<S, JitCorrect>) {
            // The lane's offset afresh from the tile's first column, which the
            // kernel left in the epilogue as a scalar: `off` kept live across
            // the main loop is the VGPR pair that k_rs_jitw_repair<J10> and
            // <J12> hold in scratch (profiles/repair_generated/)
            const long long o =
                this->tile0 + 32 * (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            const bool in = o + 32 <= a.len;
            scrub_slots<SlotsW<W::R>, NV, TPW>(static_cast<const S&>(*this), a.k, a.rows, dsts, b, r0, nrow, wave, tw,
                                               in, in ? (uint32_t)o : 0u, reinterpret_cast<uint8_t*>(lds), m4, m2,
                                               m1, this->tile0);
            return;
        }
        const bool inb = off + 32 <= a.len;
        if constexpr (S::kRepair)
            scrub_slots<SlotsW<W::R>, NV, TPW>(static_cast<const S&>(*this), a.k, a.rows, dsts, b, r0, nrow, wave, tw,
                                               inb, inb ? (uint32_t)off : 0u, reinterpret_cast<uint8_t*>(lds), m4, m2,
                                               m1, tile_start(off));
        else
            scrub_slots<SlotsW<W::R>, NV, TPW>(static_cast<const S&>(*this), a.k, a.rows, dsts, b, r0, nrow, wave, tw,
                                               inb, inb ? (uint32_t)off : 0u, reinterpret_cast<uint8_t*>(lds), m4, m2,
                                               m1);
    }
};
using JitwScrub = JitwEpi<JitScrub>;
using JitwLocate = JitwEpi<JitLocate>;
using JitwRepair = JitwEpi<JitRepair>;
using JitwCorrect = JitwEpi<JitCorrect>;

// The same decode with R rows per wave (rs_jit.h Wide): 2 waves per column
// tile; R = 16: 168 VGPRs (3 waves per SIMD), chunks of 6 sources (6
// workgroups per CU); R = 10: 120 VGPRs (4 waves per SIMD), chunks of 5 (8
// workgroups per CU).  The compiler gets v0..v39; the call clobbers
// v10..v39 and the accumulators, so what lives across it sits in v0..v8.
// hipcc warns that v129..v167 in the clobber lists are "reserved": it does
// not allocate them itself, and the kernel descriptor still gives the wave
// 168 VGPRs (.amdhsa_next_free_vgpr 168, no AGPRs), which only the asm and
// the generated code touch.
// NV = 4 (e > 32): four waves per tile, the same chunk of sources in LDS for
// all of them (rs_jit.h wide_waves / wide_row0), one tile per workgroup.
// TPW > 1 (NV = 2): one workgroup covers TPW consecutive column tiles of a block (2
// TPW waves; wave w: tile w / 2, rows of wave w % 2), so the TPW waves with
// the same rows run the same code between the same chunk barriers and share
// its instruction-cache lines.
// The body of k_rs_jitw and k_rs_jitw_scrub on block b, the block's workgroup
// wg (as jit_run): the accumulation, then the epilogue `epi` on the wave's slots.
template <class W, int TPW, int NV, class Epi>
__device__ __forceinline__ void jitw_run(const JitArgs& a, uint4 (&lds)[2][TPW][W::CS * 2 * 64], int wv, int wave,
                                         int tw, int lane, int b, long long wg, long long tile, const Epi& epi)
{
    constexpr int CS = W::CS, R = W::R;
    const int k = a.k;
    const int nch = (k + CS - 1) / CS;
    const int bw = (int)Hooks::data_block(b);
    const uint8_t* const* srcs = a.srcs + (size_t)bw * k;
    uint8_t* const* dsts = a.dsts + (size_t)bw * a.dst_stride;
    const uint8_t* code = a.code + (size_t)Hooks::code_block(b) * a.block_stride + (size_t)wave * nch * a.chunk_stride;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4*)&lds[0][tw][0];
    constexpr uint32_t kBuf = TPW * CS * 2 * 64 * 16;  // bytes between the two chunk buffers
    const long long off = Hooks::data_offset(tile * 2048 + lane * 32, tile, lane);
    // lanes past the row end re-read its head (results never stored; at C4
    // 24 of 64 lanes of every row's last tile).  Loading nothing there cut
    // the C4 decode's HBM bytes but not its time (3.26-3.28 vs 3.26-3.27 ms
    // per slice, same box x3, round 5): the head is in L2.
    const uint32_t loff = off + 32 <= a.len ? (uint32_t)off : 0u;
    if (wv == 0)
        asm volatile("s_icache_inv\n s_nop 15\n s_nop 15" ::: "memory");
    // the row pointers through the constant address space: scalar loads the
    // compiler issues together and waits for once, a chunk ahead of their
    // use (one s_load + wait per source measured 5-7 % of the wave's time)
    typedef const uint8_t* const __attribute__((address_space(4)))* CPtrs;
    const CPtrs csrcs = (CPtrs)srcs;
    constexpr int PW = (CS + NV - 1) / NV;  // this wave's sources per chunk: t = wave, wave + NV, ...
    auto ptrs = [&](int ch, const uint8_t* (&p)[PW]) {
        const int c0 = ch * CS, nt = min(CS, k - c0);
#pragma unroll
        for (int i = 0; i < PW; ++i)
            p[i] = csrcs[c0 + min(wave + NV * i, nt - 1)];  // in bounds, unconditional
    };
    // NOTE: the first word of chunk buffer 1 carries the chunk rotation
    // (below) until every wave has read it, before the first chunk barrier:
    // no LDS-DMA may target buffer 1 (par 1) before that barrier.
    auto issue = [&](int ch, int par, const uint8_t* const (&p)[PW]) {
        const int c0 = ch * CS, nt = min(CS, k - c0);
        const uint32_t base = lds0 + (uint32_t)(par * kBuf);
#pragma unroll
        for (int i = 0; i < PW; ++i) {
            const int t = wave + NV * i;
            if (t < nt) {
                if (a.code_prefetch)  // short rows: keep the block's code in L2
                    glds32_nt(p[i], loff, base + (uint32_t)(t * 2 * 64 * 16));
                else
                    glds32(p[i], loff, base + (uint32_t)(t * 2 * 64 * 16));
            }
        }
    };
    if constexpr (R == 16)
        asm volatile(RSGPU_J16_ZERO ::: RSGPU_J16_ACC_CLOBBERS);
    else if constexpr (R == 12)
        asm volatile(RSGPU_J12_ZERO ::: RSGPU_J12_ACC_CLOBBERS);
    else
        asm volatile(RSGPU_J10_ZERO ::: RSGPU_J10_ACC_CLOBBERS);
    JitwPhases ph;
    // Wave priority: a wave's transposes up to the chunk barrier run at level
    // 2 (a.prio != 0, the default) over the other waves' generated code, so
    // the workgroup's last wave reaches the barrier sooner (same process ABBA,
    // round 6, profiles/r06_prio/: C3 decode -2.5 %, C4 slices -2 %, C5 -2.4 %)
    // The chunks' order is free (each chunk's code only adds into the
    // accumulators).  A rotation by the time the workgroup starts, chunk
    // (t / kRot) % nch first, keeps the workgroups that share a CU pair's
    // instruction cache at about the same chunk of their block's code
    // (workgroups that start later begin where the others are).
    // Rounded to the nearest period, so a workgroup starts with the chunk the
    // others are about to be in (same box x3, profiles/r05_rot/: C3 decode
    // 22.53-22.58 ms at 600 ticks, 23.04-23.08 in order; 450-800 all gain;
    // one process ABBA x10: the step -0.39 ms).  Re-picking the chunk before
    // every barrier by the clock measured 0.8 ms slower than this
    // (ab_knob_rot_mode2.json).
    int rot = 0;
    if (a.chunk_rot_ticks > 0) {
        // broadcast through the first word of chunk buffer 1, which no
        // LDS-DMA writes before the first chunk barrier: a separate
        // __shared__ int made the 10-row two-tile kernel 40964 bytes, four
        // bytes too many for four workgroups per CU
        volatile int& s_rot = *(volatile int*)&lds[1][0][0];
        if (threadIdx.x == 0) {
            unsigned long long t;
            asm volatile("s_memrealtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
            const unsigned long long p = (unsigned long long)a.chunk_rot_ticks;
            s_rot = (int)(((t + p / 2) / p) % (unsigned long long)nch);
        }
        __syncthreads();
        rot = __builtin_amdgcn_readfirstlane(s_rot);
    }
    auto chunk_of = [&](int i) { return i + rot >= nch ? i + rot - nch : i + rot; };
    const uint8_t* pc[PW];
    const uint8_t* pn[PW];
    ptrs(chunk_of(0), pc);
    issue(chunk_of(0), 0, pc);
    ptrs(chunk_of(min(1, nch - 1)), pn);
    if (a.code_prefetch) {
        // the block's workgroups split its code (both row halves) and pull
        // it into L2 with vector loads, every line in flight at once, so the
        // instruction fetch, which misses line by line, finds it there; the
        // wait also covers the sources just issued, needed next anyway
        const uint8_t* cb = a.code + (size_t)b * a.block_stride;
        const long long lines = ((long long)NV * nch * a.chunk_stride) >> 7;
        const long long lo = wg * lines / gridDim.x, hi = (wg + 1) * lines / gridDim.x;
        for (long long i = lo + threadIdx.x; i < hi; i += 64 * NV * TPW) {
            uint32_t d;
            asm volatile("global_load_dword %0, %1, off\n s_waitcnt vmcnt(0)" : "=v"(d) : "v"(cb + (i << 7)) : "memory");
        }
    }
    for (int i = 0; i < nch; ++i) {
        const int ch = chunk_of(i), par = i & 1;  // the chunk, its LDS buffer
        const int nt = min(CS, k - ch * CS);
        uint4* buf = lds[par][tw];
        ph.mark(0);  // phase 0: the previous call's return .. here (loop overhead, start)
        wait_vm(0);
        ph.mark(1);  // phase 1: this chunk's LDS-DMA
        if (a.prio)
            asm volatile("s_setprio 2" ::: "memory");
        {
            // (Tried, round 5: the wave's three sources' LDS reads batched in
            // hand-allocated asm, one exposed LDS latency per chunk instead of
            // three -- the step unchanged in a same-process ABBA x10,
            // profiles/r05_energy/ab_knob_asm_transposes.json; not kept.)
            const uint32_t m4 = vconst(0x0F0F0F0Fu), m2 = vconst(0x33333333u), m1 = vconst(0x55555555u);
            for (int t = wave; t < nt && Hooks::kTransposes; t += NV) {
                uint4 u = buf[(t * 2 + 0) * 64 + lane], v = buf[(t * 2 + 1) * 64 + lane];
                uint32_t Wd[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
                tr8(Wd, m4, m2, m1);
                hook_planes<Hooks>(Wd);
                buf[(t * 2 + 0) * 64 + lane] = make_uint4(Wd[0], Wd[1], Wd[2], Wd[3]);
                buf[(t * 2 + 1) * 64 + lane] = make_uint4(Wd[4], Wd[5], Wd[6], Wd[7]);
            }
        }
        ph.mark(2);  // phase 2: transposes
        barrier_lds();
        ph.mark(3);  // phase 3: the chunk barrier
        if (a.prio)
            asm volatile("s_setprio 0" ::: "memory");
        if (i + 1 < nch)
            issue(chunk_of(i + 1), par ^ 1, pn);
        ptrs(chunk_of(min(i + 2, nch - 1)), pn);  // in flight during this chunk's code
        ph.mark(4);  // phase 4: next chunk's LDS-DMA issue, row pointers
        const uint32_t la = lds0 + (uint32_t)(par * kBuf) + lane * 16;
        const uint8_t* fn = code + (size_t)Hooks::code_chunk(ch, nt == CS) * a.chunk_stride;
        if constexpr (Hooks::kZeroValuPlanes)  // the diagnostic build's variant 3 (kernel_hooks.h)
            asm volatile("v_mov_b32 v10, 0\n v_mov_b32 v11, 0\n v_mov_b32 v12, 0\n v_mov_b32 v13, 0\n"
                         " v_mov_b32 v14, 0\n v_mov_b32 v15, 0\n v_mov_b32 v16, 0\n v_mov_b32 v17, 0"
                         ::: "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17");
        if constexpr (R == 16)
            asm volatile("s_swappc_b64 s[82:83], %[fn]"
                         :
                         : [fn] "s"(fn), "{v9}"(la)
                         : RSGPU_JW_CALL_CLOBBERS, "s82", "s83", "scc", "memory", RSGPU_J16_ACC_CLOBBERS);
        else if constexpr (R == 12)
            asm volatile("s_swappc_b64 s[82:83], %[fn]"
                         :
                         : [fn] "s"(fn), "{v9}"(la)
                         : RSGPU_JW_CALL_CLOBBERS, "s82", "s83", "scc", "memory", RSGPU_J12_ACC_CLOBBERS);
        else
            asm volatile("s_swappc_b64 s[82:83], %[fn]"
                         :
                         : [fn] "s"(fn), "{v9}"(la)
                         : RSGPU_JW_CALL_CLOBBERS, "s82", "s83", "scc", "memory", RSGPU_J10_ACC_CLOBBERS);
        ph.mark(5);  // phase 5: the generated code
    }
    epi.template run<W, TPW, NV>(a, dsts, bw, wave, tw, lane, off, &lds[0][0][0]);
    ph.mark(6);  // phase 6: output transposes and stores (the scrub: stored rows, compare)
    ph.end(wv);
}

template <class W, int TPW, int NV>
__global__ __launch_bounds__(64 * NV * TPW) __attribute__((amdgpu_num_vgpr(40))) void k_rs_jitw(JitArgs a)
{
    __shared__ uint4 lds[2][TPW][W::CS * 2 * 64];
    RSGPU_DIAG_BEGIN()
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave = wv % NV, tw = wv / NV;  // rows of the wave, its tile in the workgroup
    const int lane = threadIdx.x & 63;
    RSGPU_JIT_PLACE(a, b, wg)  // wg: this workgroup's index within its block
    const long long tile = wg * TPW + tw;
    if (a.status && a.status[b] != 0)
        return;
    jitw_run<W, TPW, NV>(a, lds, wv, wave, tw, lane, b, wg, tile, JitwStore{});
    RSGPU_DIAG_END();
}

// k_rs_jitw over [0, lo[b]) of block b, as k_rs_jit_batch: a workgroup whose
// first tile starts at or behind lo[b] leaves at once; in the others a tile
// behind lo[b] is idle as a tile behind the row end is in k_rs_jitw.
template <class W, int TPW, int NV>
__global__ __launch_bounds__(64 * NV * TPW) __attribute__((amdgpu_num_vgpr(40))) void k_rs_jitw_batch(JitArgs a,
                                                                                                     const int* lo)
{
    __shared__ uint4 lds[2][TPW][W::CS * 2 * 64];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave = wv % NV, tw = wv / NV;
    const int lane = threadIdx.x & 63;
    RSGPU_JIT_PLACE(a, b, wg)
    const int len = batch_lo(lo, b);
    if (batch_past(wg * TPW, len))
        return;
    const long long tile = wg * TPW + tw;
    JitArgs ab = a;
    ab.len = len;
    jitw_run<W, TPW, NV>(ab, lds, wv, wave, tw, lane, b, wg, tile, JitwStore{});
}

// The (64, 32) encode through the Karatsuba-split program (jit_prog.h
// build_karatsuba_code): one column tile per workgroup of three role waves
// (wave 0 = P, 1 = Q1, 2 = Q2), each in k_rs_jitw's 16-row register contract
// (168 VGPRs, 3 waves per SIMD), each accumulating one pure 16 x 32 product
// over all 8 chunks of 4 source pairs (8 real sources, 16 KB per buffer;
// double-buffered LDS-DMA, the in-place transposes, the priority window and
// the start-time chunk rotation as jitw_run).  Of a chunk's 8 transposes P
// takes 2 (positions 2, 5: it also forms the virtual sources), Q1 and Q2 3
// each (0 3 6 / 1 4 7); a wave transposes what it loaded.  After the last
// chunk P writes its 16 rows as planes over the two chunk buffers (2 x 16 KB,
// contiguous), and Q1 / Q2 run their combine chunk on them (y[r] = P[r] ^
// Q1[r], y[16 + r] = sigma_r P[r] ^ Q2[r]) and store rows 0-15 / 16-31 with
// k_rs_jitw's epilogue.
// One tile per workgroup (32 KB of LDS, four workgroups per CU, 3 waves per
// SIMD): the tiles of a CU start and end independently, so one's first loads
// and last stores run beside the others' code, and a barrier waits for three
// waves.  Measured at C3 in one process (profiles/karatsuba3/): 20.85 ms,
// against 23.10 ms for four tiles per workgroup (12 waves, 128 KB, one
// workgroup per CU) and 29.87 ms for two (six-wave workgroups spread unevenly
// over the SIMDs, as DESIGN 4 records for the decode).
__global__ __launch_bounds__(64 * 3) __attribute__((amdgpu_num_vgpr(40))) void k_rs_kara(JitArgs a)
{
    constexpr int CS = 2 * jit::kKaraPairs, NCH = jit::kKaraSrcChunks, K = 64;
    __shared__ uint4 lds[2][CS * 2 * 64];
    const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    RSGPU_JIT_PLACE(a, b, tile)
    const uint8_t* const* srcs = a.srcs + (size_t)b * K;
    uint8_t* const* dsts = a.dsts + (size_t)b * a.dst_stride;
    const uint8_t* code = a.code + (size_t)role * jit::kKaraChunks * a.chunk_stride;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4*)&lds[0][0];
    constexpr uint32_t kBuf = CS * 2 * 64 * 16;  // bytes between the two chunk buffers
    const long long off = tile * 2048 + lane * 32;
    const uint32_t loff = off + 32 <= a.len ? (uint32_t)off : 0u;  // past the row end: its head, never stored
    if (role == 0)
        asm volatile("s_icache_inv\n s_nop 15\n s_nop 15" ::: "memory");
    typedef const uint8_t* const __attribute__((address_space(4)))* CPtrs;
    const CPtrs csrcs = (CPtrs)srcs;
    const int first = role == 0 ? 2 : role - 1;  // this wave's positions of a chunk: first, first + 3, ...
    constexpr int PW = 3;
    auto ptrs = [&](int ch, const uint8_t* (&p)[PW]) {
#pragma unroll
        for (int i = 0; i < PW; ++i)
            p[i] = csrcs[jit::kara_source(ch, min(first + 3 * i, CS - 1))];  // in bounds, unconditional
    };
    // NOTE: the first word of chunk buffer 1 carries the chunk rotation until
    // every wave has read it, before the first chunk barrier: no LDS-DMA may
    // target buffer 1 before that barrier.
    auto issue = [&](int par, const uint8_t* const (&p)[PW]) {
        const uint32_t base = lds0 + (uint32_t)(par * kBuf);
#pragma unroll
        for (int i = 0; i < PW; ++i) {
            const int t = first + 3 * i;
            if (t < CS)
                glds32(p[i], loff, base + (uint32_t)(t * 2 * 64 * 16));
        }
    };
    asm volatile(RSGPU_J16_ZERO ::: RSGPU_J16_ACC_CLOBBERS);
    int rot = 0;
    if (a.chunk_rot_ticks > 0) {
        volatile int& s_rot = *(volatile int*)&lds[1][0];
        if (threadIdx.x == 0) {
            unsigned long long t;
            asm volatile("s_memrealtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
            const unsigned long long p = (unsigned long long)a.chunk_rot_ticks;
            s_rot = (int)(((t + p / 2) / p) % (unsigned long long)NCH);
        }
        __syncthreads();
        rot = __builtin_amdgcn_readfirstlane(s_rot);
    }
    auto chunk_of = [&](int i) { return i + rot >= NCH ? i + rot - NCH : i + rot; };
    const uint8_t* pc[PW];
    const uint8_t* pn[PW];
    ptrs(chunk_of(0), pc);
    issue(0, pc);
    ptrs(chunk_of(1), pn);
    for (int i = 0; i < NCH; ++i) {
        const int ch = chunk_of(i), par = i & 1;  // the chunk, its LDS buffer
        uint4* buf = lds[par];
        wait_vm(0);
        if (a.prio)
            asm volatile("s_setprio 2" ::: "memory");
        {
            const uint32_t m4 = vconst(0x0F0F0F0Fu), m2 = vconst(0x33333333u), m1 = vconst(0x55555555u);
            for (int t = first; t < CS; t += 3) {
                uint4 u = buf[(t * 2 + 0) * 64 + lane], v = buf[(t * 2 + 1) * 64 + lane];
                uint32_t Wd[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
                tr8(Wd, m4, m2, m1);
                buf[(t * 2 + 0) * 64 + lane] = make_uint4(Wd[0], Wd[1], Wd[2], Wd[3]);
                buf[(t * 2 + 1) * 64 + lane] = make_uint4(Wd[4], Wd[5], Wd[6], Wd[7]);
            }
        }
        barrier_lds();
        if (a.prio)
            asm volatile("s_setprio 0" ::: "memory");
        if (i + 1 < NCH)
            issue(par ^ 1, pn);
        ptrs(chunk_of(min(i + 2, NCH - 1)), pn);  // in flight during this chunk's code
        const uint32_t la = lds0 + (uint32_t)(par * kBuf) + lane * 16;
        const uint8_t* fn = code + (size_t)ch * a.chunk_stride;
        asm volatile("s_swappc_b64 s[82:83], %[fn]"
                     :
                     : [fn] "s"(fn), "{v9}"(la)
                     : RSGPU_JW_CALL_CLOBBERS, "s82", "s83", "scc", "memory", RSGPU_J16_ACC_CLOBBERS);
    }
    // the combine, once per tile: every wave is past the last chunk's planes,
    // P's rows replace them, Q1 and Q2 add them to their own
    barrier_lds();
    if (role == 0) {
        uint4* tb = &lds[0][0];
        [&]<int... Ss>(std::integer_sequence<int, Ss...>) {
            (
                [&] {
                    uint32_t Wd[8];
                    read_slotw<Ss>(Wd);
                    tb[(Ss * 2 + 0) * 64 + lane] = make_uint4(Wd[0], Wd[1], Wd[2], Wd[3]);
                    tb[(Ss * 2 + 1) * 64 + lane] = make_uint4(Wd[4], Wd[5], Wd[6], Wd[7]);
                }(),
                ...);
        }(std::make_integer_sequence<int, 16>{});
    }
    barrier_lds();
    if (role != 0) {
        const uint32_t la = lds0 + lane * 16;
        const uint8_t* fn = code + (size_t)NCH * a.chunk_stride;
        asm volatile("s_swappc_b64 s[82:83], %[fn]"
                     :
                     : [fn] "s"(fn), "{v9}"(la)
                     : RSGPU_JW_CALL_CLOBBERS, "s82", "s83", "scc", "memory", RSGPU_J16_ACC_CLOBBERS);
        const int half = role - 1;  // rows 16 half .. 16 half + 15 (wide_row0(32, half))
        JitwStore{}.run<jit::J16, 1, 2>(a, dsts, b, half, 0, lane, off, nullptr);
    }
}

// The generated scrub for 16 < e <= 64: k_rs_jitw's accumulation on the
// matrix's shared program, then the scrub epilogue (scrub_slots)
template <class W, int TPW, int NV>
__global__ __launch_bounds__(64 * NV * TPW) __attribute__((amdgpu_num_vgpr(40))) void k_rs_jitw_scrub(JitScrubArgs s)
{
    __shared__ uint4 lds[2][TPW][W::CS * 2 * 64];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave = wv % NV, tw = wv / NV;
    const int lane = threadIdx.x & 63;
    RSGPU_JIT_PLACE(s.j, b, wg)
    const long long tile = wg * TPW + tw;
    jitw_run<W, TPW, NV>(s.j, lds, wv, wave, tw, lane, b, wg, tile, JitwScrub{{s.fold, s.tab, s.locate}});
}

// The generated locate for 16 < e <= 64: k_rs_jitw_scrub with the span cold
// path (JitLocate above)
template <class W, int TPW, int NV>
__global__ __launch_bounds__(64 * NV * TPW) __attribute__((amdgpu_num_vgpr(40))) void k_rs_jitw_locate(JitLocateArgs s)
{
    __shared__ uint4 lds[2][TPW][W::CS * 2 * 64];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave = wv % NV, tw = wv / NV;
    const int lane = threadIdx.x & 63;
    RSGPU_JIT_PLACE(s.j, b, wg)
    const long long tile = wg * TPW + tw;
    jitw_run<W, TPW, NV>(s.j, lds, wv, wave, tw, lane, b, wg, tile,
                         JitwLocate{{s.fold, s.cand, s.cand_stride, s.slots, s.u}});
}

// The generated repair for 16 < e <= 64: k_rs_jitw_scrub with the correcting
// cold path (JitRepair above), gated as k_rs_jit_repair
template <class W, int TPW, int NV>
__global__ __launch_bounds__(64 * NV * TPW) __attribute__((amdgpu_num_vgpr(40))) void k_rs_jitw_repair(JitRepairArgs s)
{
    __shared__ uint4 lds[2][TPW][W::CS * 2 * 64];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave = wv % NV, tw = wv / NV;
    const int lane = threadIdx.x & 63;
    RSGPU_JIT_PLACE(s.j, b, wg)
    if (s.mode == kRepairGated && s.fold[b].hi1 != kRepairGate)
        return;  // uniform per workgroup
    const long long tile = wg * TPW + tw;
    jitw_run<W, TPW, NV>(s.j, lds, wv, wave, tw, lane, b, wg, tile,
                         JitwRepair{{s.fold, s.tab, s.mode, s.src, s.par, s.pitch, s.j.len}});
}

// The generated correction for 16 < e <= 64: k_rs_jitw_repair in its
// kRepairColumns mode with the pair search in its cold path (JitCorrect above)
template <class W, int TPW, int NV>
__global__ __launch_bounds__(64 * NV * TPW) __attribute__((amdgpu_num_vgpr(40))) void k_rs_jitw_correct(JitCorrectArgs s)
{
    __shared__ uint4 lds[2][TPW][W::CS * 2 * 64];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave = wv % NV, tw = wv / NV;
    const int lane = threadIdx.x & 63;
    RSGPU_JIT_PLACE(s.j, b, wg)
    const long long tile = wg * TPW + tw;
    jitw_run<W, TPW, NV>(s.j, lds, wv, wave, tw, lane, b, wg, tile,
                         JitwCorrect{{s.fold, s.tab, s.t, s.src, s.par, s.pitch, s.j.len, tile * 2048}});
}

// ---------------------------------------------------------------------------
// The degraded scrub (rsgpu_scrub_degraded_blocks under FUSED with the scrub
// kernel GENERATED; k_rs_jit_degraded, k_rs_jitw_degraded): degraded_tile
// (rs_bitsliced.hip) for a matrix known at run time, on the tables
// k_degraded_prepare wrote for the block (rs_kernels.h: the pivot parity rows
// Q, the other surviving parity rows `rest`, R and, with locate, every row's
// reduced column H).  The wave holds rows [r0, r0 + nrow) of the computed
// parity in its slots, as in scrub_slots, and what each of them is -- pivot
// i, rest row pi, or lost -- is a ballot of the row against Q (lane i: Q[i])
// and against `rest` (lane l: rest[l]), so every test below is wave-uniform.
//   barrier    other waves may still be reading the last chunk's planes; the
//              header, the row pointers and the first pivot row's load are
//              under way before it
//   pivots     the stored row (one row's load in flight ahead), tr8, the
//              slot's planes XORed in: the syndrome s_Q[i], written to pivot
//              slot i of the wave's tile ([2][64] uint4 = 2 KB, at most 8,
//              behind the masks); a barrier
//   rest rows  the stored row likewise, then t_p = s_p ^ XOR_i R[p][i] s_Q[i],
//              the pivot's planes read once per i and multiplied by the
//              uniform constant on planes (plane_mul.h); the OR over the rest
//              rows' planes is the lane's mask.  xor_into leaves the slots as
//              they are, so they hold the computed parity to the end and
//              nothing is kept across the pivot barrier
//   lost rows  neither loaded nor counted; their pointers may be loaded
// A surviving parity row's 32 bytes per lane are so loaded once.  From the
// masks on, scrub_slots' logic: the masks meet in LDS (their 2 KiB part is no
// pivot slot's), a clean workgroup ends there and has written nothing, wave 0
// of a bad tile counts the tile's bad columns.
// The cold path (a dirty workgroup with locate; small code, not fast code) is
// the generated scrub's eight passes: the waves lay 4 bytes per lane of the
// raw syndromes of the surviving parity rows into LDS (syn [e][256] per tile,
// over the pivot slots, which every wave is past at the mask barrier; zeros
// for a lost row, which is not loaded), and a tile's threads walk the 256
// columns on bytes: a column with a non-zero syndrome is reduced in place, by
// the one thread that owns it, and judged by deg_locate's rule
// (degraded_column_row below).
// LDS, in the chunk buffers: masks 2 KiB | per tile 8 pivot slots of 2 KiB,
// then syn [e][256] in their place.
// ---------------------------------------------------------------------------
constexpr int kDegSlotBytes = 2 * 64 * 16, kDegSlots = 8;

struct JitDegraded {
    ScrubFold* fold;
    const uint8_t* tab;  // the block's own table
    int locate;
    long long tile0 = 0;  // k_rs_jitw_degraded: the first column of the wave's tile (JitwDeg)
};

// deg_locate's rule (rs_degraded.hip) on the reduced syndromes t(p), p <
// nrest, of one bad column: the first non-zero entry p*, a screen on one other
// entry, then t_p h_r[p*] == t_p* h_r[p] for every rest row; a row only when
// exactly one of the k + e rows passes (H of a lost row is zero).  h: the
// table's H, [rows][e].  A second copy of what degraded_tile (rs_bitsliced.hip)
// walks: that one runs on compile-time K and E and its own LDS layout, and
// sharing the text changes k_rs_bs_degraded's code, which this form leaves as
// it is.
template <class T>
__device__ __forceinline__ int degraded_column_row(int rows, int e, int nrest, const uint8_t* h, T&& t)
{
    auto mul = [](uint8_t a, uint8_t b) -> uint8_t { return a && b ? kGfJit.exp[kGfJit.log[a] + kGfJit.log[b]] : 0; };
    int ps = -1;
    uint8_t ts = 0, t0 = 0, t2 = 0;
#pragma unroll 1
    for (int p = 0; p < nrest; ++p) {
        const uint8_t v = t(p);
        if (p == 0)
            t0 = v;
        if (ps < 0 && v) {
            ps = p;
            ts = v;
        } else if (ps >= 0 && p == ps + 1) {
            t2 = v;
        }
    }
    if (ps < 0)
        return -2;  // not a bad column
    // the screen: entry 0 (zero) when p* > 0, else entry 1 when there is one
    const int p2 = ps > 0 ? 0 : nrest > 1 ? 1 : -1;
    if (ps > 0)
        t2 = t0;
    int found = 0, row = -1;
#pragma unroll 1
    for (int r = 0; r < rows && found < 2; ++r) {
        const uint8_t* hr = h + (size_t)r * e;
        const uint8_t hs = hr[ps];
        if (!hs)
            continue;
        if (p2 >= 0 && mul(t2, hs) != mul(ts, hr[p2]))
            continue;
        bool ok = true;
#pragma unroll 1
        for (int p = 0; p < nrest && ok; ++p)
            ok = mul(t(p), hs) == mul(ts, hr[p]);
        if (ok) {
            ++found;
            row = r;
        }
    }
    return found == 1 ? row : -1;
}

template <class SL, int NV, int TPW>
__device__ __forceinline__ void degraded_slots(const JitDegraded& s, int k, int e, uint8_t* const* dsts, int b, int r0,
                                               int nrow, int wave, int tw, bool inb, uint32_t po, uint8_t* ldsb,
                                               uint32_t m4, uint32_t m2, uint32_t m1)
{
    static_assert(4 * NV * TPW * 64 <= kScrubMaskBytes, "the masks fit their part");
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    // the block's table: the header, and R[pi] per rest row below, through the
    // constant address space (scalar registers); lane l < e rest[l]
    const uint8_t* tab = s.tab;
    const uint8_t* t_rest = tab + sizeof(DegradedHdr);
    const uint8_t* t_r = t_rest + degraded_rest_bytes(e);
    typedef const uint32_t __attribute__((address_space(4))) * CHdr;
    const uint32_t hd1 = ((CHdr)tab)[1], hd2 = ((CHdr)tab)[2], hd3 = ((CHdr)tab)[3];
    const int nq = (int)(hd1 & 0xFFu), nrest = (int)((hd1 >> 8) & 0xFFu);
    // Q and `rest` ascend and the wave's rows are consecutive, so its pivots
    // take consecutive slots and its rest rows consecutive indices: two bit
    // masks (bit i: row r0 + i) and the first of each, in scalar registers
    unsigned pivm = 0, restm = 0;
    int slot0 = 0, pi0 = 0;
    {
        const int rv = lane < e ? ((const g_cu8*)t_rest)[lane] : 0;
        const int qv = (int)(((lane & 4 ? hd3 : hd2) >> (8 * (lane & 3))) & 0xFFu);  // lane i < 8: Q[i]
        const unsigned long long qlanes = (1ull << nq) - 1;  // nq <= 8
        const unsigned long long rlanes = nrest >= 64 ? ~0ull : (1ull << nrest) - 1;
#pragma unroll
        for (int i = SL::N - 1; i >= 0; --i) {
            const int sq = __ffsll(__ballot(qv == r0 + i) & qlanes), sr = __ffsll(__ballot(rv == r0 + i) & rlanes);
            if (i < nrow) {
                pivm |= (sq ? 1u : 0u) << i;
                restm |= (sr ? 1u : 0u) << i;
                slot0 = sq ? sq - 1 : slot0;
                pi0 = sr ? sr - 1 : pi0;
            }
        }
    }
    // the row's pivot slot / index among the rest rows, as 1 + index, 0: none
    auto pivot_of = [&](int i) { return (pivm >> i) & 1u ? 1 + slot0 + __builtin_popcount(pivm & ((1u << i) - 1)) : 0; };
    auto rest_of = [&](int i) { return (restm >> i) & 1u ? 1 + pi0 + __builtin_popcount(restm & ((1u << i) - 1)) : 0; };
    // the stored rows' pointers: scalar loads under one wait, clamped in bounds
    typedef const uint8_t* const __attribute__((address_space(4)))* CRows;
    const uint8_t* dp[SL::N];
#pragma unroll
    for (int i = 0; i < SL::N; ++i)
        dp[i] = ((CRows)dsts)[min(r0 + i, e - 1)];
    uint4* piv = reinterpret_cast<uint4*>(ldsb + kScrubMaskBytes + tw * (kDegSlots * kDegSlotBytes));
    uint32_t Pn[8];
    bs::load32(dp[0], po, pivot_of(0) != 0, Pn);
    __syncthreads();  // the chunk buffers are free
    [&]<int... Ss>(std::integer_sequence<int, Ss...>) {
        (
            [&] {
                if (Ss < nrow) {
                    const int slot = pivot_of(Ss);
                    uint32_t Pw[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        Pw[q] = Pn[q];
                    if constexpr (Ss + 1 < SL::N)
                        if (Ss + 1 < nrow)
                            bs::load32(dp[Ss + 1], po, pivot_of(Ss + 1) != 0, Pn);
                    if (slot) {
                        tr8(Pw, m4, m2, m1);
                        SL::template xor_into<Ss>(Pw);  // the pivot's syndrome, as planes
                        piv[((slot - 1) * 2 + 0) * 64 + lane] = make_uint4(Pw[0], Pw[1], Pw[2], Pw[3]);
                        piv[((slot - 1) * 2 + 1) * 64 + lane] = make_uint4(Pw[4], Pw[5], Pw[6], Pw[7]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }(),
            ...);
    }(std::make_integer_sequence<int, SL::N>{});
    bs::load32(dp[0], po, rest_of(0) != 0, Pn);
    __syncthreads();  // the pivots' syndromes are in their slots
    uint32_t mine = 0;
    [&]<int... Ss>(std::integer_sequence<int, Ss...>) {
        (
            [&] {
                if (Ss < nrow) {
                    const int pi = rest_of(Ss);
                    uint32_t Pw[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        Pw[q] = Pn[q];
                    if constexpr (Ss + 1 < SL::N)
                        if (Ss + 1 < nrow)
                            bs::load32(dp[Ss + 1], po, rest_of(Ss + 1) != 0, Pn);
                    if (pi) {
                        // R[pi]: byte i the factor of pivot i, a scalar load under the transpose
                        const uint32_t f0 = nq ? ((CHdr)t_r)[2 * (pi - 1)] : 0u,
                                       f1 = nq > 4 ? ((CHdr)t_r)[2 * (pi - 1) + 1] : 0u;
                        tr8(Pw, m4, m2, m1);
                        SL::template xor_into<Ss>(Pw);  // the syndrome, as planes
#pragma unroll 1
                        for (int i = 0; i < nq; ++i) {
                            const uint32_t c = ((i & 4 ? f1 : f0) >> (8 * (i & 3))) & 0xFFu;
                            if (c) {
                                const uint4 u = piv[(i * 2 + 0) * 64 + lane], v = piv[(i * 2 + 1) * 64 + lane];
                                const uint32_t sq[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
                                plane_mul_acc(Pw, sq, c);
                            }
                        }
#pragma unroll
                        for (int q = 0; q < 8; ++q)
                            mine |= Pw[q];
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }(),
            ...);
    }(std::make_integer_sequence<int, SL::N>{});
    uint32_t* wmask = reinterpret_cast<uint32_t*>(ldsb);
    wmask[(tw * NV + wave) * 64 + lane] = inb ? mine : 0u;
    __syncthreads();
    uint32_t tm = 0, any = 0;  // this lane's columns: of the tile, of the workgroup
#pragma unroll
    for (int g = 0; g < NV * TPW; ++g) {
        const uint32_t m = wmask[g * 64 + lane];
        any |= m;
        tm |= g / NV == tw ? m : 0u;
    }
    if (__ballot(any != 0) == 0)
        return;  // the same for every wave of the workgroup
    ScrubFold* f = s.fold + b;
    if (wave == 0) {
        unsigned n = __builtin_popcount(tm);
        for (int o = 32; o > 0; o >>= 1)
            n += __shfl_down(n, o, 64);
        if (lane == 0 && n)
            atomicAdd(&f->bad, (unsigned long long)n);
    }
    if (!s.locate)
        return;
    // as scrub_slots' cold path: LDS through its own address space, the stored
    // dword through an SGPR base and one VGPR offset, every loop rolled
    typedef __attribute__((address_space(3))) uint8_t lds_u8;
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    lds_u8* syn = (lds_u8*)ldsb + kScrubMaskBytes + tw * e * 256;
    const uint8_t* t_h = t_r + (size_t)e * 8;
    const unsigned live = pivm | restm;  // bit i: row r0 + i survives
    unsigned hi1 = 0, lo1 = 0;
    auto mul = [](uint8_t x, uint8_t y) -> uint8_t { return x && y ? kGfJit.exp[kGfJit.log[x] + kGfJit.log[y]] : 0; };
#pragma unroll 1
    for (int pass = 0; pass < 8; ++pass) {
        // bytes 4 pass .. 4 pass + 3 of the lane's 32 of every row (zeros from an idle lane)
        lds_u32* mine4 = (lds_u32*)(syn + r0 * 256 + lane * 4);
        const uint32_t po4 = po + 4 * pass;
        const uint32_t p4 = vconst(0x0F0F0F0Fu), p2 = vconst(0x33333333u), p1 = vconst(0x55555555u);
        [&]<int... Ss>(std::integer_sequence<int, Ss...>) {
            (
                [&] {
                    if (Ss < nrow) {
                        uint32_t d = 0;
                        if ((live >> Ss) & 1u) {
                            uint32_t W[8], st;
                            // (s_nop 4: as scrub_slots)
                            asm volatile("s_nop 4\n global_load_dword %0, %1, %2\n s_waitcnt vmcnt(0)"
                                         : "=v"(st)
                                         : "v"(po4), "s"(dp[Ss])
                                         : "memory");
                            SL::template read<Ss>(W);
                            tr8(W, p4, p2, p1);  // computed parity, bytes
                            d = W[0];
#pragma unroll
                            for (int q = 1; q < 8; ++q)
                                d = pass == q ? W[q] : d;
                            d ^= st;
                        }
                        mine4[Ss * 64] = inb ? d : 0u;
                        __builtin_amdgcn_sched_barrier(0);  // slot by slot
                    }
                }(),
                ...);
        }(std::make_integer_sequence<int, SL::N>{});
        __syncthreads();
#pragma unroll 1
        for (int c = wave * 64 + lane; c < 256; c += 64 * NV) {
            unsigned nz = 0;
#pragma unroll 1
            for (int p = 0; p < e; ++p)
                nz |= syn[p * 256 + c];
            if (!nz)
                continue;  // no surviving row's syndrome: t is zero
            // t_p over s_p, in place: the column is this thread's alone
#pragma unroll 1
            for (int p = 0; p < nrest; ++p) {
                lds_u8* at = syn + t_rest[p] * 256 + c;
                uint8_t t = *at;
#pragma unroll 1
                for (int i = 0; i < nq; ++i)
                    t ^= mul(t_r[p * 8 + i], syn[((i & 4 ? hd3 : hd2) >> (8 * (i & 3)) & 0xFFu) * 256 + c]);
                *at = t;
            }
            const int row = degraded_column_row(k + e, e, nrest, t_h, [&](int p) { return syn[t_rest[p] * 256 + c]; });
            if (row == -2)
                continue;  // consistent: the pivots' syndromes explain it
            hi1 = max(hi1, row >= 0 ? (unsigned)row + 1 : kScrubNoRow);
            lo1 = max(lo1, row >= 0 ? kScrubBias - (unsigned)row : kScrubNoRow);
        }
        __syncthreads();  // the next pass overwrites syn
    }
    for (int o = 32; o > 0; o >>= 1) {
        hi1 = max(hi1, (unsigned)__shfl_down((int)hi1, o, 64));
        lo1 = max(lo1, (unsigned)__shfl_down((int)lo1, o, 64));
    }
    if (lane == 0 && hi1) {
        atomicMax(&f->hi1, hi1);
        atomicMax(&f->lo1, lo1);
    }
}

// the state k_degraded_prepare left in a block's table, in a scalar register
__device__ __forceinline__ int degraded_state(const uint8_t* tab)
{
    return *(const int __attribute__((address_space(4)))*)tab;
}

// wave w's rows [8 w, 8 w + 8) of k_rs_jit's layout ...
struct JitDeg8 : JitDegraded {
    template <int NW>
    __device__ __forceinline__ void run(const JitArgs& a, uint8_t* const* dsts, int b, int wave, int,
                                        long long off, uint4* lds, uint32_t m4, uint32_t m2, uint32_t m1) const
    {
        static_assert(kScrubMaskBytes + kDegSlots * kDegSlotBytes <= 2 * C * 2 * 64 * 16 &&
                          kScrubMaskBytes + 32 * 256 <= 2 * C * 2 * 64 * 16,
                      "masks and pivot slots, then masks and syn (rows <= 32), fit the chunk buffers");
        const bool inb = off + 32 <= a.len;
        degraded_slots<Slots8, NW, 1>(static_cast<const JitDegraded&>(*this), a.k, a.rows, dsts, b, wave * 8,
                                      min(8, a.rows - wave * 8), wave, 0, inb, inb ? (uint32_t)off : 0u,
                                      reinterpret_cast<uint8_t*>(lds), m4, m2, m1);
    }
};

// ... and the wave's rows of k_rs_jitw's (JitwEpi)
struct JitwDeg : JitDegraded {
    template <class W, int TPW, int NV>
    __device__ __forceinline__ void run(const JitArgs& a, uint8_t* const* dsts, int b, int wave, int tw, int,
                                        long long, uint4* lds) const
    {
        static_assert(kScrubMaskBytes + TPW * kDegSlots * kDegSlotBytes <= 2 * TPW * W::CS * 2 * 64 * 16,
                      "masks and every tile's pivot slots fit the chunk buffers");
        static_assert(kScrubMaskBytes + TPW * (NV == 4 ? 64 : 32) * 256 <= 2 * TPW * W::CS * 2 * 64 * 16,
                      "e <= 32 (two waves), e <= 64 (four): syn fits the chunk buffers");
        const uint32_t m4 = vconst(0x0F0F0F0Fu), m2 = vconst(0x33333333u), m1 = vconst(0x55555555u);
        const int r0 = jit::wide_row0(a.rows, wave), nrow = jit::wide_row0(a.rows, wave + 1) - r0;
        // the lane's offset afresh from the tile's first column, a scalar (as
        // JitwEpi does for the correction): `off` kept live across the main
        // loop put a VGPR of these kernels into scratch
        const long long o =
            this->tile0 + 32 * (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const bool inb = o + 32 <= a.len;
        degraded_slots<SlotsW<W::R>, NV, TPW>(static_cast<const JitDegraded&>(*this), a.k, a.rows, dsts, b, r0, nrow,
                                              wave, tw, inb, inb ? (uint32_t)o : 0u,
                                              reinterpret_cast<uint8_t*>(lds), m4, m2, m1);
    }
};

// The generated degraded scrub for e <= 16: k_rs_jit<NW, true>'s accumulation
// on the matrix's shared program, then degraded_slots.  A workgroup whose
// block the prepare has already reported (state != kDegRun) leaves before it
// touches a row pointer or LDS; the test is uniform per workgroup.
template <int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_num_vgpr(64))) void k_rs_jit_degraded(JitDegradedArgs s)
{
    __shared__ uint4 lds[2][C * 2 * 64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    RSGPU_JIT_PLACE(s.j, b, tile)
    const uint8_t* tab = s.tab + (size_t)b * s.tab_stride;
    if (degraded_state(tab) != kDegRun)
        return;
    jit_run<NW, true, JitHooks>(s.j, lds, wave, lane, b, tile, JitDeg8{{s.fold, tab, s.locate}});
}

// ... and for 16 < e <= 64, on k_rs_jitw's
template <class W, int TPW, int NV>
__global__ __launch_bounds__(64 * NV * TPW) __attribute__((amdgpu_num_vgpr(40))) void k_rs_jitw_degraded(JitDegradedArgs s)
{
    __shared__ uint4 lds[2][TPW][W::CS * 2 * 64];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave = wv % NV, tw = wv / NV;
    const int lane = threadIdx.x & 63;
    RSGPU_JIT_PLACE(s.j, b, wg)
    const uint8_t* tab = s.tab + (size_t)b * s.tab_stride;
    if (degraded_state(tab) != kDegRun)
        return;
    const long long tile = wg * TPW + tw;
    jitw_run<W, TPW, NV>(s.j, lds, wv, wave, tw, lane, b, wg, tile, JitwDeg{{s.fold, tab, s.locate, tile * 2048}});
}

// every 8-byte slot a return: a call that lands in code never written
// comes straight back
__global__ void k_jit_fill(uint64_t* code, long long n)
{
    const uint64_t ret = (uint64_t)jit::S_NOP0 << 32 | jit::S_SETPC_82;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x)
        code[i] = ret;
}

RSGPU_DIAG_READER(diag_read_jitw)
RSGPU_DIAG_PHASE_READER(diag_read_jitw_phase)

}  // namespace jitk

// One workgroup per (block, wave), the wave's rows of the block's matrix
// staged in LDS first: a thread per (source, slot) writes that coefficient's
// eight multiply-accumulate words (one 64-byte run, consecutive threads
// consecutive runs), a thread per preamble word, then the chunks' ends.
// Layout as rs_jit.h describes; the words are those of jit::code_word (the
// host emitter the CPU suite interprets).  (Earlier forms: emission inside
// the prepare kernel, 0.41 ms at C3; one workgroup per (block, wave, chunk),
// dispatch-bound at 0.49 ms; one thread per word with the index arithmetic
// and the coefficient's matrix recomputed per word, 0.19 ms.)
__global__ __launch_bounds__(256) void k_jit_emit(int k, int e, const uint8_t* coef, const int* status,
                                                  uint8_t* code)
{
    __shared__ uint8_t cw[8 * 256];  // rows 8 w .. 8 w + 7 (k <= 250)
    const int b = blockIdx.y, w = blockIdx.x;
    if (status[b] != 0)
        return;
    const int nw = (e + 7) / 8, nch = (k + 7) / 8;
    const int nslot = min(8, e - 8 * w);
    const size_t stride = (size_t)jit::chunk_stride(8);
    uint8_t* cbase = code + ((size_t)b * nw + w) * nch * stride;
    const int sb = jit::src_bytes(nslot);
    for (int i = threadIdx.x; i < nslot * k; i += blockDim.x)
        cw[i] = coef[((size_t)b * e + 8 * w) * k + i];
    __syncthreads();
    for (int i = threadIdx.x; i < 8 * k; i += blockDim.x) {
        const int q = i >> 3, s = i & 7;
        if (s >= nslot)
            continue;
        const int ch = q >> 3, t = q & 7;
        uint64_t wd[8];
        jit::mac_words(cw[s * k + q], s, t & 1, wd);
        uint4* dst = reinterpret_cast<uint4*>(cbase + (size_t)ch * stride + jit::PRO_BYTES + (size_t)t * sb +
                                              jit::PRE_BYTES + 64 * s);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            dst[j] = make_uint4((uint32_t)wd[2 * j], (uint32_t)(wd[2 * j] >> 32), (uint32_t)wd[2 * j + 1],
                                (uint32_t)(wd[2 * j + 1] >> 32));
    }
    constexpr int PW = jit::PRE_BYTES / 8;  // preamble words per source
    for (int i = threadIdx.x; i < PW * k; i += blockDim.x) {
        const int q = i / PW, r = i - q * PW;
        const int ch = q >> 3, t = q & 7, nt = min(8, k - 8 * ch);
        reinterpret_cast<uint64_t*>(cbase + (size_t)ch * stride + jit::PRO_BYTES + (size_t)t * sb)[r] =
            (uint64_t)jit::pre_u32(t, nt, 2 * r + 1) << 32 | jit::pre_u32(t, nt, 2 * r);
    }
    for (int i = threadIdx.x; i < 3 * nch; i += blockDim.x) {  // prologue words, return
        const int ch = i / 3, o = i - 3 * ch, nt = min(8, k - 8 * ch);
        uint64_t word;
        (void)jit::code_word(cw, k, nslot, ch, o < 2 ? o : 2 + nt * (PW + 8 * nslot), &word);
        reinterpret_cast<uint64_t*>(cbase + (size_t)ch * stride)[o < 2 ? o : 2 + nt * (PW + 8 * nslot)] = word;
    }
}

// The word tables of k_jitw_emit (rs_jit.h wide_tables), built at compile time.
__constant__ jit::WideTables kWideTab = jit::wide_tables();

// k_rs_jitw<R>'s code (rs_jit.h Wide), one workgroup per (block, wave) as
// k_jit_emit: rows wide_row0(e, w) .. wide_row0(e, w + 1) - 1 of the block's decode rows.  Each word
// is a table entry (the coefficient's matrix row and register operands are
// fixed per (c, plane)) with the accumulator ORed in: per 16 bytes of code
// one 16-byte table load, two selects and ORs.  (Computing every word from
// the coefficient's 8 x 8 matrix took ~3500 VALU + 2400 SALU per wave; the
// emission of a C4 batch, 2.5 GB of code, 0.85-0.9 ms.)
// e > 64: one launch per pass of the rows (rs_jit.h wide_passes), rows
// row_base .. row_base + rows - 1 of the block's e decode rows, the pass's code
// at pass_off in each block's block_stride bytes.
template <class W>
__global__ __launch_bounds__(256) void k_jitw_emit(int k, int e, int row_base, int rows, long long block_stride,
                                                   long long pass_off, const uint8_t* coef, const int* status,
                                                   uint8_t* code)
{
    constexpr int R = W::R, CS = W::CS, PW = W::PRE / 8;
    static_assert(PW == jit::WideTables::PW && CS <= 6, "preamble table: PW words per source, chunk positions < 6");
    __shared__ uint8_t cw[R * 256];
    const int b = blockIdx.y, w = blockIdx.x;
    if (status[b] != 0)
        return;
    const int nch = (k + CS - 1) / CS;
    const int r0 = row_base + jit::wide_row0(rows, w), nslot = jit::wide_row0(rows, w + 1) - jit::wide_row0(rows, w);
    const size_t stride = (size_t)W::chunk_stride();
    uint8_t* cbase = code + (size_t)b * block_stride + pass_off + (size_t)w * nch * stride;
    const int sb = W::src_bytes(nslot);
    // every load of a phase in flight before its first use: the loops below
    // would otherwise wait a full memory latency per iteration
    {
        const uint8_t* cr = coef + ((size_t)b * e + r0) * k;
        constexpr int NB = R * 256 / 256;  // bytes per thread, nslot * k <= R * 250
        uint8_t v[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int i = threadIdx.x + 256 * j;
            v[j] = i < nslot * k ? cr[i] : 0;
        }
#pragma unroll
        for (int j = 0; j < NB; ++j)
            cw[threadIdx.x + 256 * j] = v[j];
    }
    __syncthreads();
    // (source, slot) runs of 64 bytes, one 16-byte quarter (planes 2j, 2j+1)
    // per thread, so a wave's store covers 1 KB of consecutive code; U table
    // loads issued together
    constexpr int U = 8;
    for (int i0 = threadIdx.x; i0 < R * k * 4; i0 += 256 * U) {
        uint4 bw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + 256 * u, run = i >> 2, q = run / R, s = run - q * R;
            const int c = i < R * k * 4 && s < nslot ? cw[s * k + q] : 0;
            bw[u] = *reinterpret_cast<const uint4*>(&kWideTab.mac[8 * c + 2 * (i & 3)]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + 256 * u, run = i >> 2, j = i & 3, q = run / R, s = run - q * R;
            if (i >= R * k * 4 || s >= nslot)
                continue;
            const int ch = q / CS, t = q - ch * CS;
            const int acc = W::ACC + 8 * s + 2 * j;
            const uint64_t w0 = W::with_acc((uint64_t)bw[u].y << 32 | bw[u].x, acc);
            const uint64_t w1 = W::with_acc((uint64_t)bw[u].w << 32 | bw[u].z, acc + 1);
            reinterpret_cast<uint4*>(cbase + (size_t)ch * stride + (size_t)t * sb + W::PRE + 64 * s)[j] =
                make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
        }
    }
    // preambles: this thread's words of the table are fixed by its index mod 14
    for (int i0 = threadIdx.x; i0 < PW * k; i0 += 256 * 4) {
        uint64_t pw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + 256 * u, q = i / PW, r = i - q * PW, t = q % CS;
            pw[u] = kWideTab.pre[i < PW * k ? PW * t + r : 0];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + 256 * u, q = i / PW, r = i - q * PW;
            if (i >= PW * k)
                continue;
            const int ch = q / CS, t = q - ch * CS;
            reinterpret_cast<uint64_t*>(cbase + (size_t)ch * stride + (size_t)t * sb)[r] = pw[u];
        }
    }
    for (int ch = threadIdx.x; ch < nch; ch += blockDim.x) {  // returns
        const int nt = min(CS, k - CS * ch);
        reinterpret_cast<uint64_t*>(cbase + (size_t)ch * stride)[nt * (PW + 8 * nslot)] =
            (uint64_t)jit::S_NOP0 << 32 | jit::S_SETPC_82;
    }
}

// rows per wave of the 2-wave layout for e rows, 0 = the 8-row layout
// (e > 64: the layout of each pass, jitw_pass_rows)
int jitw_rows(int e)
{
    if (e > 32)  // four waves
        return e > 48 && e <= 64 ? 16 : e > 40 && e <= 64 ? 12 : e > 32 && e <= 64 ? 10 : 0;
    return e > 24 ? 16 : e > 20 ? 12 : e > 16 ? 10 : 0;
}

int jitw_rot_ticks(int rows)
{
    // one chunk's work per wave, CS (8 R + 24) VALU, times the waves sharing
    // a SIMD (4 for the 10-row kernels, 3 otherwise), scaled from C3's
    // measured optimum (R 16, CS 6, 3 waves: 600 ticks).  C5 (R 10): 456;
    // 500 measured 0.6 % faster than 342 and 200 1.1 % slower
    // (profiles/r05_rot/c5_period.json); 456 against 342 same process ABBA
    // x6: -0.14 ms per C5 step (c5_period_456_vs_342.json)
    const int r = jitw_rows(rows), cs = jitw_cs(rows), waves = r == 10 ? 4 : 3;
    return r ? 600 * cs * (8 * r + 24) * waves / (6 * (8 * 16 + 24) * 3) : 0;
}

int jitw_cs(int e) { return jitw_rows(e) == 16 ? jit::J16::CS : jitw_rows(e) == 12 ? jit::J12::CS : jit::J10::CS; }

size_t jitw_chunk_stride(int e)
{
    const int r = jitw_rows(e);
    return r == 16 ? jit::J16::chunk_stride() : r == 12 ? jit::J12::chunk_stride() : jit::J10::chunk_stride();
}

// the layout covers e: 16 < e <= 64 in one launch, 64 < e <= 125 in passes
bool jitw_layout(int e)
{
    return e > 16 && (e <= 64 || (e <= 128 && jitw_rows(jit::wide_pass_rows(e, 0)) &&
                                                        jitw_rows(jit::wide_pass_rows(e, jit::wide_passes(e) - 1))));
}

// one block's code of a pass of `rows` (<= 64) rows
size_t jitw_pass_bytes(int k, int rows)
{
    const int cs = jitw_cs(rows);
    return (size_t)jit::wide_waves(rows) * ((k + cs - 1) / cs) * jitw_chunk_stride(rows);
}

size_t jitw_pass_offset(int k, int e, int p)
{
    size_t o = 0;
    for (int q = 0; q < p; ++q)
        o += jitw_pass_bytes(k, jit::wide_pass_rows(e, q));
    return o;
}

size_t jitw_code_bytes(int k, int e, long long blocks)
{
    return (size_t)blocks * jitw_pass_offset(k, e, jit::wide_passes(e));
}

hipError_t launch_jitw_emit(int k, int e, long long blocks, const uint8_t* coef, const int* status,
                            uint8_t* code, hipStream_t st)
{
    if (k <= 0 || k > 250 || !jitw_layout(e) || k + e > 250 || blocks <= 0 || !coef || !status || !code)
        return hipErrorInvalidValue;
    const long long bs = (long long)jitw_code_bytes(k, e, 1);
    for (int p = 0; p < jit::wide_passes(e); ++p) {
        const int r0 = jit::wide_pass_row0(e, p), rows = jit::wide_pass_rows(e, p);
        const long long off = (long long)jitw_pass_offset(k, e, p);
        const dim3 grid(jit::wide_waves(rows), (unsigned)blocks);
        if (jitw_rows(rows) == 16)
            hipLaunchKernelGGL(k_jitw_emit<jit::J16>, grid, dim3(256), 0, st, k, e, r0, rows, bs, off, coef, status, code);
        else if (jitw_rows(rows) == 12)
            hipLaunchKernelGGL(k_jitw_emit<jit::J12>, grid, dim3(256), 0, st, k, e, r0, rows, bs, off, coef, status, code);
        else
            hipLaunchKernelGGL(k_jitw_emit<jit::J10>, grid, dim3(256), 0, st, k, e, r0, rows, bs, off, coef, status, code);
    }
    return hipGetLastError();
}

hipError_t launch_rs_jitw(const JitArgs& a, long long blocks, hipStream_t st)
{
    if (!jitw_rows(a.rows) || a.dst_stride < a.rows || a.k <= 0 || !a.code || a.chunk_stride <= 0)
        return hipErrorInvalidValue;
    // four waves per tile (e > 32): one tile per workgroup, three 4-wave
    // workgroups fill a CU's 12 wave slots
    const int nv = jit::wide_waves(a.rows);
    const int tpw = nv == 4 ? 1 : a.tiles_per_wg >= 3 ? 3 : a.tiles_per_wg == 2 ? 2 : 1;
    const long long ntile = (a.len + 2047) / 2048;
    dim3 grid((unsigned)((ntile + tpw - 1) / tpw), (unsigned)blocks);
    dim3 blk(64 * nv * tpw);
#define RSGPU_JW_LAUNCH(WT)                                                                          \
    if (nv == 4)                                                                                     \
        hipLaunchKernelGGL((jitk::k_rs_jitw<WT, 1, 4>), grid, blk, 0, st, a);                        \
    else                                                                                             \
        switch (tpw) {                                                                               \
        case 3: hipLaunchKernelGGL((jitk::k_rs_jitw<WT, 3, 2>), grid, blk, 0, st, a); break;        \
        case 2: hipLaunchKernelGGL((jitk::k_rs_jitw<WT, 2, 2>), grid, blk, 0, st, a); break;        \
        default: hipLaunchKernelGGL((jitk::k_rs_jitw<WT, 1, 2>), grid, blk, 0, st, a); break;       \
        }
    if (jitw_rows(a.rows) == 16) {
        RSGPU_JW_LAUNCH(jit::J16)
    } else if (jitw_rows(a.rows) == 12) {
        RSGPU_JW_LAUNCH(jit::J12)
    } else {
        RSGPU_JW_LAUNCH(jit::J10)
    }
#undef RSGPU_JW_LAUNCH
    return hipGetLastError();
}

hipError_t launch_rs_kara(const JitArgs& a, long long blocks, hipStream_t st)
{
    if (a.k != 64 || a.rows != 32 || a.dst_stride < 32 || !a.code || a.chunk_stride <= 0 || a.len <= 0 ||
        a.len % 32 || blocks <= 0 || blocks > (long long)kMaxGridBlocks)
        return hipErrorInvalidValue;
    const long long ntile = (a.len + 2047) / 2048;
    hipLaunchKernelGGL(jitk::k_rs_kara, dim3((unsigned)ntile, (unsigned)blocks), dim3(64 * 3), 0, st, a);
    return hipGetLastError();
}

size_t jit_code_bytes(int k, int e, long long blocks)
{
    const int nw = (e + 7) / 8, nch = (k + 7) / 8;
    return (size_t)blocks * nw * nch * jit::chunk_stride(8);
}

hipError_t launch_jit_fill(void* code, size_t bytes, hipStream_t st)
{
    hipLaunchKernelGGL(jitk::k_jit_fill, dim3(4096), dim3(256), 0, st, (uint64_t*)code,
                       (long long)(bytes / 8));
    return hipGetLastError();
}

hipError_t launch_jit_emit(int k, int e, long long blocks, const uint8_t* coef, const int* status,
                           uint8_t* code, hipStream_t st)
{
    if (k <= 0 || k > 250 || e <= 0 || k + e > 250 || blocks <= 0 || !coef || !status || !code)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_jit_emit, dim3((unsigned)((e + 7) / 8), (unsigned)blocks), dim3(256), 0, st, k, e,
                       coef, status, code);
    return hipGetLastError();
}

__global__ void k_jit_copy(uint64_t* dst, const uint64_t* src, long long n)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

// up to PutArgs::kWords 8-byte words from the kernel arguments to device
// memory: a small upload (a call's row pointers) without a host staging
// buffer, its copy and the host's wait for the previous one
__global__ void k_put_words(PutArgs a)
{
    if ((int)threadIdx.x < a.n)
        a.dst[threadIdx.x] = a.w[threadIdx.x];
}

hipError_t launch_put_words(void* dst, const void* src, size_t bytes, hipStream_t st)
{
    if (bytes % 8 || bytes > sizeof(PutArgs::w) || !dst)
        return hipErrorInvalidValue;
    PutArgs a{};
    a.dst = (uint64_t*)dst;
    a.n = (int)(bytes / 8);
    std::memcpy(a.w, src, bytes);
    hipLaunchKernelGGL(k_put_words, dim3(1), dim3(PutArgs::kWords), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_jit_copy(void* dst, const void* src, size_t bytes, hipStream_t st)
{
    if (bytes % 8)
        return hipErrorInvalidValue;
    const long long n = (long long)(bytes / 8);
    const unsigned grid = (unsigned)std::min<long long>(1024, (n + 255) / 256);
    hipLaunchKernelGGL(k_jit_copy, dim3(grid), dim3(256), 0, st, (uint64_t*)dst, (const uint64_t*)src, n);
    return hipGetLastError();
}

hipError_t launch_rs_jit(const JitArgs& a, long long blocks, hipStream_t st)
{
    if (a.rows <= 0 || a.rows > 32 || a.dst_stride < a.rows || a.k <= 0 || !a.code || a.chunk_stride <= 0)
        return hipErrorInvalidValue;
    const int nw = (a.rows + 7) / 8;
    dim3 grid((unsigned)((a.len + 2047) / 2048), (unsigned)blocks);
    const bool sh = a.block_stride == 0;
    switch (nw * 2 + (sh ? 1 : 0)) {
    case 2: hipLaunchKernelGGL((jitk::k_rs_jit<1, false>), grid, dim3(64), 0, st, a); break;
    case 3: hipLaunchKernelGGL((jitk::k_rs_jit<1, true>), grid, dim3(64), 0, st, a); break;
    case 4: hipLaunchKernelGGL((jitk::k_rs_jit<2, false>), grid, dim3(128), 0, st, a); break;
    case 5: hipLaunchKernelGGL((jitk::k_rs_jit<2, true>), grid, dim3(128), 0, st, a); break;
    case 6: hipLaunchKernelGGL((jitk::k_rs_jit<3, false>), grid, dim3(192), 0, st, a); break;
    case 7: hipLaunchKernelGGL((jitk::k_rs_jit<3, true>), grid, dim3(192), 0, st, a); break;
    case 8: hipLaunchKernelGGL((jitk::k_rs_jit<4, false>), grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((jitk::k_rs_jit<4, true>), grid, dim3(256), 0, st, a); break;
    }
    return hipGetLastError();
}

// launch_rs_jit's (shared program) and launch_rs_jitw's choice of kernel and
// tiles per workgroup, on the entries with a length per block
hipError_t launch_rs_jit_batch(const JitArgs& a, bool wide, const int* lo, long long max_lo, long long blocks,
                               hipStream_t st)
{
    if (a.rows <= 0 || a.rows > 64 || a.dst_stride < a.rows || a.k <= 0 || !a.code || a.chunk_stride <= 0 ||
        a.block_stride != 0 || !lo || max_lo <= 0 || max_lo % 32 || max_lo > 0x7fffffffLL || blocks <= 0 ||
        blocks > (long long)kMaxGridBlocks)
        return hipErrorInvalidValue;
    const long long ntile = (max_lo + 2047) / 2048;
    if (!wide) {  // the 8-row layout
        if (a.rows > 32)
            return hipErrorInvalidValue;
        dim3 grid((unsigned)ntile, (unsigned)blocks);
        switch ((a.rows + 7) / 8) {
        case 1: hipLaunchKernelGGL((jitk::k_rs_jit_batch<1>), grid, dim3(64), 0, st, a, lo); break;
        case 2: hipLaunchKernelGGL((jitk::k_rs_jit_batch<2>), grid, dim3(128), 0, st, a, lo); break;
        case 3: hipLaunchKernelGGL((jitk::k_rs_jit_batch<3>), grid, dim3(192), 0, st, a, lo); break;
        default: hipLaunchKernelGGL((jitk::k_rs_jit_batch<4>), grid, dim3(256), 0, st, a, lo); break;
        }
        return hipGetLastError();
    }
    if (!jitw_rows(a.rows))
        return hipErrorInvalidValue;
    const int nv = jit::wide_waves(a.rows);
    const int tpw = nv == 4 ? 1 : a.tiles_per_wg >= 3 ? 3 : a.tiles_per_wg == 2 ? 2 : 1;
    dim3 grid((unsigned)((ntile + tpw - 1) / tpw), (unsigned)blocks);
    dim3 blk(64 * nv * tpw);
#define RSGPU_JWB_LAUNCH(WT)                                                                            \
    if (nv == 4)                                                                                        \
        hipLaunchKernelGGL((jitk::k_rs_jitw_batch<WT, 1, 4>), grid, blk, 0, st, a, lo);                 \
    else                                                                                                \
        switch (tpw) {                                                                                  \
        case 3: hipLaunchKernelGGL((jitk::k_rs_jitw_batch<WT, 3, 2>), grid, blk, 0, st, a, lo); break; \
        case 2: hipLaunchKernelGGL((jitk::k_rs_jitw_batch<WT, 2, 2>), grid, blk, 0, st, a, lo); break; \
        default: hipLaunchKernelGGL((jitk::k_rs_jitw_batch<WT, 1, 2>), grid, blk, 0, st, a, lo); break; \
        }
    if (jitw_rows(a.rows) == 16) {
        RSGPU_JWB_LAUNCH(jit::J16)
    } else if (jitw_rows(a.rows) == 12) {
        RSGPU_JWB_LAUNCH(jit::J12)
    } else {
        RSGPU_JWB_LAUNCH(jit::J10)
    }
#undef RSGPU_JWB_LAUNCH
    return hipGetLastError();
}

// The grids and the kernel choice of launch_rs_jit (shared program) and
// launch_rs_jitw, on the three kernel families that end in scrub_slots.
namespace {

struct ScrubFamily {
    using Args = JitScrubArgs;
    template <int NW>
    static constexpr auto jit = &jitk::k_rs_jit_scrub<NW>;
    template <class W, int TPW, int NV>
    static constexpr auto wide = &jitk::k_rs_jitw_scrub<W, TPW, NV>;
};
struct LocateFamily {
    using Args = JitLocateArgs;
    template <int NW>
    static constexpr auto jit = &jitk::k_rs_jit_locate<NW>;
    template <class W, int TPW, int NV>
    static constexpr auto wide = &jitk::k_rs_jitw_locate<W, TPW, NV>;
};

struct RepairFamily {
    using Args = JitRepairArgs;
    template <int NW>
    static constexpr auto jit = &jitk::k_rs_jit_repair<NW>;
    template <class W, int TPW, int NV>
    static constexpr auto wide = &jitk::k_rs_jitw_repair<W, TPW, NV>;
};

struct CorrectFamily {
    using Args = JitCorrectArgs;
    template <int NW>
    static constexpr auto jit = &jitk::k_rs_jit_correct<NW>;
    template <class W, int TPW, int NV>
    static constexpr auto wide = &jitk::k_rs_jitw_correct<W, TPW, NV>;
};

struct DegradedFamily {
    using Args = JitDegradedArgs;
    template <int NW>
    static constexpr auto jit = &jitk::k_rs_jit_degraded<NW>;
    template <class W, int TPW, int NV>
    static constexpr auto wide = &jitk::k_rs_jitw_degraded<W, TPW, NV>;
};

template <class F, class W>
void launch_wide(const typename F::Args& s, int nv, int tpw, dim3 grid, dim3 blk, hipStream_t st)
{
    if (nv == 4)
        hipLaunchKernelGGL((F::template wide<W, 1, 4>), grid, blk, 0, st, s);
    else if (tpw == 3)
        hipLaunchKernelGGL((F::template wide<W, 3, 2>), grid, blk, 0, st, s);
    else if (tpw == 2)
        hipLaunchKernelGGL((F::template wide<W, 2, 2>), grid, blk, 0, st, s);
    else
        hipLaunchKernelGGL((F::template wide<W, 1, 2>), grid, blk, 0, st, s);
}

template <class F>
hipError_t launch_scrub_family(const typename F::Args& s, long long blocks, hipStream_t st)
{
    const JitArgs& a = s.j;
    if (a.rows <= 0 || a.rows > 64 || a.dst_stride < a.rows || a.k <= 0 || !a.code || a.chunk_stride <= 0 ||
        a.block_stride != 0 || a.status || a.len <= 0 || a.len % 32 || a.len >= (1LL << 32) || blocks <= 0 ||
        blocks > (long long)kMaxGridBlocks || !s.fold)
        return hipErrorInvalidValue;
    const long long ntile = (a.len + 2047) / 2048;
    if (!jitw_rows(a.rows)) {  // e <= 16
        dim3 grid((unsigned)ntile, (unsigned)blocks);
        if (a.rows <= 8)
            hipLaunchKernelGGL((F::template jit<1>), grid, dim3(64), 0, st, s);
        else
            hipLaunchKernelGGL((F::template jit<2>), grid, dim3(128), 0, st, s);
        return hipGetLastError();
    }
    const int nv = jit::wide_waves(a.rows);
    const int tpw = nv == 4 ? 1 : a.tiles_per_wg >= 3 ? 3 : a.tiles_per_wg == 2 ? 2 : 1;
    dim3 grid((unsigned)((ntile + tpw - 1) / tpw), (unsigned)blocks);
    dim3 blk(64 * nv * tpw);
    if (jitw_rows(a.rows) == 16)
        launch_wide<F, jit::J16>(s, nv, tpw, grid, blk, st);
    else if (jitw_rows(a.rows) == 12)
        launch_wide<F, jit::J12>(s, nv, tpw, grid, blk, st);
    else
        launch_wide<F, jit::J10>(s, nv, tpw, grid, blk, st);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_rs_jit_scrub(const JitScrubArgs& s, long long blocks, hipStream_t st)
{
    if (s.locate && !s.tab)
        return hipErrorInvalidValue;
    return launch_scrub_family<ScrubFamily>(s, blocks, st);
}

// writable rows a block of k (e) rows apart, as the row pointers of s.j name them
hipError_t launch_rs_jit_repair(const JitRepairArgs& s, long long blocks, hipStream_t st)
{
    if (!s.tab || !s.src || !s.par || s.pitch < s.j.len || s.mode < kRepairLocate || s.mode > kRepairColumns)
        return hipErrorInvalidValue;
    return launch_scrub_family<RepairFamily>(s, blocks, st);
}

// The chunk buffers hold the search's tables (jitk::CorLds): always but for
// the four waves of 16 rows per tile (48 < e <= 64, one tile per workgroup, 24
// KiB), where masks, syn, PairGf and four waves' CorRow [k] come to 3336 +
// 256 e + 32 k bytes.  The other layouts fit at every k + e <= 250, which their
// epilogues assert.
bool jit_correct_fits(int k, int e, int t)
{
    if (t != 2)
        return true;
    if (jit::wide_waves(e) == 4 && jitw_rows(e) == 16)
        return jitk::CorLds<4, 1>::bytes(k, e) <= 2 * jit::J16::CS * 2 * 64 * 16;
    return true;
}

// rows as launch_rs_jit_repair's; t == 2 needs the three syndromes the search
// screens at, a lane per syndrome, and the tables in LDS
hipError_t launch_rs_jit_correct(const JitCorrectArgs& s, long long blocks, hipStream_t st)
{
    if (!s.tab || !s.src || !s.par || s.pitch < s.j.len || s.j.k + s.j.rows > 250 ||
        !((s.t == 1 && s.j.rows >= 3) || (s.t == 2 && s.j.rows >= 5 && s.j.rows <= 64)) ||
        !jit_correct_fits(s.j.k, s.j.rows, s.t))
        return hipErrorInvalidValue;
    return launch_scrub_family<CorrectFamily>(s, blocks, st);
}

// the blocks' tables as k_degraded_prepare wrote them, 16-byte aligned
hipError_t launch_rs_jit_degraded(const JitDegradedArgs& s, long long blocks, hipStream_t st)
{
    if (!s.tab || (uintptr_t)s.tab % 16 || s.tab_stride % 16 || s.tab_stride < degraded_tab_stride(s.j.k, s.j.rows))
        return hipErrorInvalidValue;
    return launch_scrub_family<DegradedFamily>(s, blocks, st);
}

// a slot per tile: no workgroup's claim can pass the block's area
hipError_t launch_rs_jit_locate(const JitLocateArgs& s, long long blocks, hipStream_t st)
{
    if (!s.cand || s.u < 1 || s.u > kLocMax || s.slots < (s.j.len + 2047) / 2048 ||
        s.cand_stride < (size_t)s.slots * kLocateSlotBytes)
        return hipErrorInvalidValue;
    return launch_scrub_family<LocateFamily>(s, blocks, st);
}

}  // namespace rsgpu
