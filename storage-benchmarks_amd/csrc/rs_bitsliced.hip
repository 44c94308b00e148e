// rs_bitsliced.hip -- bit-sliced RS(K, E) parity kernel with
// compile-time coefficients (the gf_gen_rs_matrix code, isa/ec_base.c:62-79).
//
// Why bit-slicing: on gfx950 a wave64 v_bitop3/v_xor/v_and issues in ~2
// cycles per SIMD but v_perm/v_pk_*/v_bfi in ~4 (profiles/r1_ubench_valu.log),
// and the GF(2^8) product by a constant is GF(2)-linear.  With each lane
// holding 32 consecutive bytes of a row as 8 bit-planes (plane a = bit a of
// the 32 bytes), multiplying by a constant c and accumulating is, per output
// plane, one 3-input XOR of two "four Russians" entries
//     out_b ^= L[m_b & 15] ^ H[m_b >> 4],
// L[n] = XOR of planes 0..3 selected by n, H[n] = same for planes 4..7, m_b =
// row b of c's 8x8 bit matrix.  That is 8 full-rate ops per (coefficient,
// 32 bytes) versus 24 quarter-rate v_perm for the same bytes.  With the
// coefficients known at compile time, only the composites a block of rows
// actually uses are built (gen_enc_progs.py: a greedy cover, 10.9 instead of
// 22 per source on average; the encode measured 2.7 % faster).
//
// Code size: the parity matrix has entries 2^(r*j).  Sources are processed in
// chunks of C with Horner's rule over chunks,
//     p_r = sum_c 2^(C r c) * E_c(r),   E_c(r) = sum_t 2^(r t) d_{cC+t},
// so one chunk's straight-line code (coefficients 2^(r t), t < C) serves
// every chunk; between chunks each accumulator is multiplied by the constant
// 2^(C r) (~16 XORs).  The chunk loop is a runtime loop.  A chunk's source 0
// has the coefficient 1 on every row: its single-plane terms ride along in
// the 3-input XOR of a later source whose term is a single value too
// (T0Pair, gen_enc_progs.py), 3 % fewer instructions at (64, 32).
//
// Work split: a workgroup of NW waves shares 64 x 32 = 2048 byte positions;
// wave w owns outputs [w*OPW, (w+1)*OPW) (8 planes x OPW accumulators in
// VGPRs, <= 128 VGPRs for 4 waves/SIMD).  The NW waves divide each chunk's
// sources for loading + transposing into LDS, then all read every source's
// planes from LDS.  Bit transposes are SWAR 8x8 bit-matrix transposes across
// the lane's 8 dwords (12 block swaps), and the same routine converts the
// accumulators back to bytes.
//
// The parity scrub of these codes (k_rs_bs_scrub) is the same accumulation
// with another epilogue: the stored parity read and compared in registers
// instead of the computed one written (scrub_tile).  The repair
// (k_rs_bs_repair) is that epilogue with the rows writable: a bad column's
// byte is corrected where its row and error value are found.  The locate of
// several rows (k_rs_bs_locate) is the scrub with another cold path: a dirty
// tile leaves the span of its syndrome columns (span_tile).  The degraded scrub
// (k_rs_bs_degraded) reduces the syndromes of a block with known-lost rows on
// planes before the mask (degraded_tile).
//
// The compiled codes are the generator's list (RSGPU_BS_PLANS in
// enc_progs.inc); with_plan, at the end of the file, is the one dispatch from
// a call's (k, e) to its plan, for every launcher and every query.
//
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "bitslice.h"
#include "diag_clock.h"
#include "gf256.h"
#include "kernel_hooks.h"
#include "plane_mul.h"
#include "rs_kernels.h"
#include "rs_pairs.h"
#include "rs_span.h"

namespace rsgpu {
namespace bs {

RSGPU_DIAG_TABLE

template <int K, int E, int C>
struct PlanHolder {  // the code (K, E) and its Horner chunk C
    static constexpr int k = K, e = E, c = C;
};

// Per-source XOR programs (gen_enc_progs.py -> build/enc_progs.inc): for
// rows R0..R0+NR-1 at chunk position T, the composite XORs of the source
// planes that the block's masks need (values 8..), and for every output
// plane the one or two values it adds.
template <int K, int E, int C, int R0, int NR, int T>
struct EncProg;
template <int K, int E, int C, int R>
struct TwProg;
template <int K, int E, int C, int R0, int NR>
struct T0Pair;
#include "enc_progs.inc"

template <class PR, int I, int NV>
__device__ __forceinline__ void prog_op(uint32_t (&V)[NV]);

// row R's accumulator times 2^(C R): the generated XOR program over its 8
// planes (TwProg, gen_enc_progs.py)
template <class P, int R, int... Bs>
__device__ __forceinline__ void twiddle_row(uint32_t (&acc)[8], std::integer_sequence<int, Bs...>)
{
    using PR = TwProg<P::k, P::e, P::c, R>;
    uint32_t V[8 + PR::NOPS];
#pragma unroll
    for (int a = 0; a < 8; ++a)
        V[a] = acc[a];
    [&]<int... Is>(std::integer_sequence<int, Is...>) {
        (prog_op<PR, Is>(V), ...);
    }(std::make_integer_sequence<int, PR::NOPS>{});
    ((acc[Bs] = V[PR::outs[Bs]]), ...);
}

template <class P, int R0, int NR, int... Rs>
__device__ __forceinline__ void twiddle_rows(uint32_t (&acc)[NR][8], std::integer_sequence<int, Rs...>)
{
    (twiddle_row<P, R0 + Rs>(acc[Rs], std::make_integer_sequence<int, 8>{}), ...);
}

template <class PR, int I, int NV>
__device__ __forceinline__ void prog_op(uint32_t (&V)[NV])
{
    constexpr int a = PR::ops[I][0], b = PR::ops[I][1], c = PR::ops[I][2];
    if constexpr (c == 255)
        V[8 + I] = V[a] ^ V[b];
    else
        V[8 + I] = x3(V[a], V[b], V[c]);
}

// Output O of source T: its one or two values; source 0's single plane
// moves to the partner source of T0Pair (one 3-input XOR for both terms)
template <class PR, class PP, bool PAIR, int T, int O, int NV>
__device__ __forceinline__ void prog_out(uint32_t& acc, const uint32_t (&V)[NV], const uint32_t (&p0)[8])
{
    constexpr int x = PR::outs[O][0], y = PR::outs[O][1];
    constexpr int partner = PAIR ? PP::partner[O] : 0;  // 0: source 0 adds its own plane
    if constexpr (T == 0 && partner != 0) {
        // added by source `partner`
    } else if constexpr (T != 0 && partner == T) {
        static_assert(x != 255 && y == 255, "T0 partner output must be a single value");
        acc = x3(acc, V[x], p0[O % 8]);
    } else if constexpr (x != 255 && y != 255) {
        acc = x3(acc, V[x], V[y]);
    } else if constexpr (x != 255) {
        acc ^= V[x];
    }
}

// consume source T of the chunk from planes p (all lanes), for this wave's
// rows: the generated program's composites, then one XOR per output plane
// (p0: the chunk's source 0 planes, for the outputs paired with it)
template <class P, int R0, int NR, int T, bool PAIR = true>
__device__ __forceinline__ void consume(uint32_t (&acc)[NR][8], const uint32_t (&p)[8], const uint32_t (&p0)[8])
{
    using PR = EncProg<P::k, P::e, P::c, R0, NR, T>;
    using PP = T0Pair<P::k, P::e, P::c, R0, NR>;
    constexpr int NV = 8 + PR::NOPS;
    uint32_t V[NV];
#pragma unroll
    for (int a = 0; a < 8; ++a)
        V[a] = p[a];
    [&]<int... Is>(std::integer_sequence<int, Is...>) {
        (prog_op<PR, Is>(V), ...);
    }(std::make_integer_sequence<int, PR::NOPS>{});
    [&]<int... Os>(std::integer_sequence<int, Os...>) {
        (prog_out<PR, PP, PAIR, T, Os>(acc[Os / 8][Os % 8], V, p0), ...);
    }(std::make_integer_sequence<int, NR * 8>{});
}

struct Args {
    static constexpr bool kScrub = false;  // run_group's epilogue stores the parity rows
    const uint8_t* src;   // [B][K] rows
    uint8_t* out;         // [B][E] rows
    long long pitch, len;
    long long blocks;     // B
    int flat;             // tiles over the blocks' rows laid end to end (short rows)
    int prio;             // A/B: wave priority level from the transposes to the part barrier
};

// Where lane `lane` of column tile `tile` works: the tile's first block b0,
// the lane's block b0 + db and byte offset o in its rows, and whether it has
// bytes at all.  Per block, tiles cover [0, len) in 2 KB steps, the last one
// partial (C4: 32000 = 15 x 2048 + 1280, 2.4 % of the tiles' lanes idle).
// flat: tiles cover the B blocks' rows as one run of B x len bytes per row
// index (len % 32 == 0, so a lane's 32 bytes never straddle two blocks) and
// a tile's lanes may belong to consecutive blocks: one idle tail per launch.
struct TilePos {
    long long b0, o;
    int db;
    bool inb;
};
template <class A>
__device__ __forceinline__ TilePos tile_pos(const A& a, int lane)
{
    TilePos p;
    if (!a.flat) {
        p.b0 = blockIdx.y;
        p.o = (long long)blockIdx.x * 2048 + lane * 32;
        p.db = 0;
        p.inb = p.o + 32 <= a.len;
        return p;
    }
    const long long t0 = (long long)blockIdx.x * 2048;
    p.b0 = t0 / a.len;                                // wave-uniform
    const int x = (int)(t0 - p.b0 * a.len) + lane * 32;  // < len + 2048 < 2^24
    int db = (int)((float)x * (1.0f / (float)a.len));
    const int L = (int)a.len;
    if (x - db * L >= L)
        ++db;
    if (x - db * L < 0)
        --db;
    p.db = db;
    p.o = x - (long long)db * L;
    p.inb = p.b0 + db < a.blocks;
    return p;
}

// LDS part: S sources of [2 halves][64 lanes] x 16 B; two parts double-buffer
// the source stream (2 x 16 KiB).  A plan chunk of C sources is ceil(C/S)
// consecutive parts.
constexpr int S = 8;

// Sources T = PART*S + t (t < S, T < C) of the current chunk from the LDS part.
template <class P, int K, int C, int R0, int NR, int PART>
__device__ __forceinline__ void consume_part(uint32_t (&acc)[NR][8], uint32_t (&p0)[8], const uint4* buf,
                                             int lane, int j0)
{
    [[maybe_unused]] uint32_t zp[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // kernel_hooks.h kZeroValuPlanes only
    [&]<int... Ts>(std::integer_sequence<int, Ts...>) {
        (
            [&] {
                constexpr int T = PART * S + Ts;
                if constexpr (T < C) {
                    if (j0 + Ts < K) {
                        const uint4 u = buf[(Ts * 2 + 0) * 64 + lane];
                        const uint4 v = buf[(Ts * 2 + 1) * 64 + lane];
                        uint32_t pl[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
                        if constexpr (Hooks::kZeroValuPlanes) {
                            // the reads kept, the VALU fed zeros that are new values to
                            // the compiler per source (no instruction, no CSE)
                            asm volatile("" ::"v"(u.x), "v"(u.y), "v"(u.z), "v"(u.w), "v"(v.x), "v"(v.y), "v"(v.z),
                                         "v"(v.w));
                            asm volatile("" : "+v"(zp[0]), "+v"(zp[1]), "+v"(zp[2]), "+v"(zp[3]), "+v"(zp[4]),
                                         "+v"(zp[5]), "+v"(zp[6]), "+v"(zp[7]));
#pragma unroll
                            for (int a = 0; a < 8; ++a)
                                pl[a] = zp[a];
                        }
                        if constexpr (T == 0) {
#pragma unroll
                            for (int a = 0; a < 8; ++a)
                                p0[a] = pl[a];
                        }
                        consume<P, R0, NR, T>(acc, pl, p0);
                    }
                    // keep the next source's LDS reads from being hoisted
                    // here (they would pin 8 more VGPRs per source)
                    __builtin_amdgcn_sched_barrier(0);
                }
            }(),
            ...);
    }(std::make_integer_sequence<int, S>{});
}

// ---------------------------------------------------------------------------
// Parity scrub of the compiled codes (rsgpu_scrub_blocks, k_rs_bs_scrub):
// run_group's accumulation, then this epilogue in place of the parity store.
// One workgroup per (tile, block), never the flat layout: everything a
// workgroup reduces belongs to one block.
struct ScrubArgs {
    static constexpr bool kScrub = true;
    static constexpr bool kDegraded = false;
    static constexpr bool kRepair = false;  // scrub_tile only reads the rows
    static constexpr bool kSpan = false;    // its cold path names one row per column
    static constexpr int flat = 0;
    const uint8_t* src;  // [B][K] rows
    const uint8_t* par;  // [B][E] rows, the stored parity
    long long pitch, len;
    long long blocks;
    ScrubFold* fold;  // [B], zeroed before the launch (rs_kernels.h)
    int locate;
};

// The locate of several rows (rsgpu_locate_blocks, k_rs_bs_locate): the
// scrub's arguments, and where a dirty tile leaves the span of its syndrome
// columns (rs_kernels.h launch_rs_bitsliced_locate).
struct LocArgs {
    static constexpr bool kScrub = true;
    static constexpr bool kDegraded = false;
    static constexpr bool kRepair = false;
    static constexpr bool kSpan = true;  // scrub_tile's cold path is span_tile
    static constexpr int flat = 0;
    static constexpr int locate = 1;
    const uint8_t* src;  // [B][K] rows
    const uint8_t* par;  // [B][E] rows, the stored parity
    long long pitch, len;
    long long blocks;
    ScrubFold* fold;     // [B], zeroed before the launch; hi1 counts the block's claimed slots
    uint8_t* cand;       // [B] candidate areas at cand_stride, a slot per tile
    size_t cand_stride;
    int u;
};

// The repair (rsgpu_repair_blocks, k_rs_bs_repair): the scrub's arguments
// with writable rows, the 24-byte fold and a mode (rs_kernels.h kRepair*).
struct RepairArgs {
    static constexpr bool kScrub = true;
    static constexpr bool kDegraded = false;
    static constexpr bool kRepair = true;  // scrub_tile corrects what it locates
    static constexpr bool kSpan = false;
    static constexpr int flat = 0;
    static constexpr int locate = 1;
    uint8_t* src;  // [B][K] rows
    uint8_t* par;  // [B][E] rows, the stored parity
    long long pitch, len;
    long long blocks;
    RepairFold* fold;  // [B]: zeroed (kRepairLocate, kRepairColumns) or the final reports (kRepairGated)
    int mode;
};

// The degraded scrub (rsgpu_scrub_degraded_blocks under FUSED,
// k_rs_bs_degraded): the scrub's arguments and the tables k_degraded_prepare
// wrote (rs_kernels.h DegradedHdr); the epilogue is degraded_tile.
struct DegArgs {
    static constexpr bool kScrub = true;
    static constexpr bool kDegraded = true;
    static constexpr int flat = 0;
    const uint8_t* src;  // [B][K] rows, the lost ones as they lie in memory
    const uint8_t* par;  // [B][E] rows, the stored parity; a lost row is never read
    long long pitch, len;
    long long blocks;
    const uint8_t* tab;  // [B] tables at degraded_tab_stride(K, E)
    ScrubFold* fold;  // [B]: the reports, zeroed by the prepare where the block runs
    int locate;
};

// The correction per column (rsgpu_correct_blocks under FUSED,
// k_rs_bs_correct): the repair's arguments in its kRepairColumns mode with the
// 32-byte fold, and t; with t == 2 scrub_tile's walk hands the columns no row
// explains to correct_pending.
struct CorrectArgs {
    static constexpr bool kScrub = true;
    static constexpr bool kDegraded = false;
    static constexpr bool kRepair = true;
    static constexpr bool kSpan = false;
    static constexpr int flat = 0;
    static constexpr int locate = 1;
    static constexpr int mode = kRepairColumns;
    uint8_t* src;  // [B][K] rows
    uint8_t* par;  // [B][E] rows, the stored parity
    long long pitch, len;
    long long blocks;
    CorrectFold* fold;  // [B], zeroed before the launch (rs_kernels.h)
    int t;              // 1, or 2 (E >= 5)
};

// log / antilog tables of the cold paths (the scrub's row location, the
// small-batch decode's solve below)
alignas(16) __device__ const GfTables kGfBs = make_gf_tables();

// scrub_tile's cold path of the locate (LocArgs): instead of one row per bad
// column, the span of the tile's syndrome columns (rs_span.h), as
// k_locate_span keeps it of its columns.  The syndrome planes go back to bytes
// and in four passes into LDS as the scrub's do, at a row stride of 520 bytes:
// lane p of a wave reads syndrome p of one column, and at 512 every lane of a
// half-wave would meet the same bank (520 = 130 dwords: 2 lanes per bank, the
// 8-byte writes still aligned).  After a pass's barrier the waves divide the
// tile lanes that have a bad column in it (`tm`, the tile's bad-byte masks:
// bit 8 q + w is byte 4 w + q, so column j of the pass is bit 8 (j % 4) +
// 2 pass + j / 4); each wave visits its columns one after the other, all 64
// lanes on each, under wave-uniform control, and reduces them against its own
// basis of at most u vectors.  After the last pass's barrier wave 0 merges the
// NW bases and writes them to the next free slot of the block's candidate
// area, claimed with an atomicAdd on the fold's hi1, which the locate uses for
// nothing else: a clean tile writes nothing and claims nothing, so the first
// hi1 slots of a block are the written ones and k_locate_finish reads no
// other.  The order of the claims is that of the workgroups' arrival; W, the
// span of all the block's syndrome columns, does not depend on the order in
// which its vectors are met, so no byte of the output does.
// LDS, in the part buffers: masks 1 KiB | syn [E][520] | GF tables 768 B | NW
// bases of 552 B.
constexpr int kSpanRow = 520;
template <int E, int NW, int G, int R0, int NR>
__device__ __forceinline__ void span_tile(const LocArgs& a, uint32_t (&acc)[NR][8], bool inb, uint32_t tm,
                                          long long blk, int lane, uint8_t* ldsb, uint32_t m4, uint32_t m2,
                                          uint32_t m1)
{
    constexpr int kGfAt = 1024 + E * kSpanRow, kBasesAt = kGfAt + (int)sizeof(GfTables);
    static_assert(NW == 1 || NW == 2 || NW == 4, "the waves divide the tile's 64 lanes");
    static_assert(kGfAt % 8 == 0 && sizeof(GfTables) % 8 == 0, "the bases are aligned");
    static_assert(kBasesAt + NW * sizeof(SpanBasis) <= 2 * S * 2 * 64 * 16, "locate LDS fits the part buffers");
    uint8_t* syn = ldsb + 1024;
    GfTables& gf = *reinterpret_cast<GfTables*>(ldsb + kGfAt);
    SpanBasis* sb = reinterpret_cast<SpanBasis*>(ldsb + kBasesAt);
    SpanBasis& s = sb[G];
    load_gf(gf, kGfBs, G * 64 + lane, 64 * NW);  // read from the first pass's barrier on
    s.n = 0;
    s.ovf = 0;
#pragma unroll
    for (int rr = 0; rr < NR; ++rr)
        tr8(acc[rr], m4, m2, m1);  // syndrome planes -> bytes, in place
    // tile lanes G, G + NW, ... are this wave's
    constexpr unsigned long long kShare = NW == 1 ? ~0ull : NW == 2 ? 0x5555555555555555ull : 0x1111111111111111ull;
    for (int pass = 0; pass < 4; ++pass) {
        // the lane's bytes 8 pass .. 8 pass + 7 of every row (zeros from an idle
        // lane): always the row's first two dwords, the later ones move down
        // behind the pass (register moves; an index by `pass` would put the
        // syndromes into scratch)
#pragma unroll
        for (int rr = 0; rr < NR; ++rr)
            *reinterpret_cast<uint2*>(syn + (R0 + rr) * kSpanRow + lane * 8) =
                inb ? make_uint2(acc[rr][0], acc[rr][1]) : make_uint2(0u, 0u);
#pragma unroll
        for (int rr = 0; rr < NR; ++rr)
#pragma unroll
            for (int q = 0; q < 6; ++q)
                acc[rr][q] = acc[rr][q + 2];
        __syncthreads();
        unsigned pm = 0;  // bit j: column 8 lane + j of the pass is bad
#pragma unroll
        for (int j = 0; j < 8; ++j)
            pm |= ((tm >> (8 * (j & 3) + 2 * pass + (j >> 2))) & 1u) << j;
        unsigned long long todo = __ballot(pm != 0) & (kShare << G);
        while (todo) {
            const int from = __ffsll(todo) - 1;
            todo &= todo - 1;
            unsigned m = (unsigned)__builtin_amdgcn_readlane((int)pm, from);
            while (m) {
                const int c = from * 8 + __ffs(m) - 1;
                m &= m - 1;
                const uint8_t v = lane < E ? syn[lane * kSpanRow + c] : (uint8_t)0;
                span_append(s, gf, lane, span_reduce(s, gf, lane, v), a.u);
            }
        }
        __syncthreads();  // the next pass overwrites syn; the last one: the bases are complete
    }
    if constexpr (G == 0) {
        unsigned at = 0;
        if (lane == 0)
            at = atomicAdd(&a.fold[blk].hi1, 1u);
        at = (unsigned)uni((int)at);
        if (at < gridDim.x)  // a slot per tile: always, with hi1 zero before the launch
            span_publish(s, sb, NW, gf, lane, a.u,
                         a.cand + (size_t)blk * a.cand_stride + (size_t)at * kLocateSlotBytes);
    }
}

// scrub_tile's cold path of the correction with t == 2 (CorrectArgs): the bad
// columns of a step of the walk that no row explains (`pend`, a lane each; the
// lanes of a wave walk 64 consecutive columns, lane 0 column c0) go to the
// wave one at a time, all 64 lanes on each, under wave-uniform control, with
// the pass's syndromes still in LDS.  The search is rs_correct.hip's for the
// compiled codes' own coefficients, 2^(p r) (rs_pairs.h): nothing of the matrix
// is read from memory.  The lanes' matches are counted, up to two; the lane
// that holds the only one XORs both bytes into the global rows, column c of
// pass `pass` being byte 8 pass + c % 8 of tile lane c / 8 as in the walk.
// In place for scrub_tile's reasons: the syndromes are in LDS, no byte of
// global memory is read twice.  Returns the columns corrected (0 or more,
// the same in every lane).
// LDS, in the part buffers: masks 1 KiB | syn [E][520] | PairGf (1288 B, the
// workgroup's, correct_tables) | per wave CorRow [K] and the column's
// syndromes [64].
template <int E>
constexpr int kCorGfAt = 1024 + E * kSpanRow;
template <int K>
constexpr int kCorWaveBytes = K * (int)sizeof(CorRow) + 64;
template <int K, int E, int G>
constexpr int kCorWaveAt = kCorGfAt<E> + ((int)sizeof(PairGf) + 7) / 8 * 8 + G * kCorWaveBytes<K>;


template <int E, int NW>
__device__ __forceinline__ void correct_tables(const CorrectArgs& a, uint8_t* ldsb, int tid)
{
    for (int i = tid; i < (int)sizeof(PairGf); i += 64 * NW)
        ldsb[kCorGfAt<E> + i] = pair_gf_byte(kGfBs, i);
}

template <int K, int E, int NW, int G>
__device__ __forceinline__ unsigned correct_pending(const CorrectArgs& a, bool pend, int c0, int pass, long long wb,
                                                    int lane, uint8_t* ldsb)
{
    static_assert(E >= 3 && E <= 64 && K <= 255, "a lane per syndrome; 2^r distinct over the data rows");
    static_assert(kCorGfAt<E> % 8 == 0 && kCorWaveBytes<K> % 8 == 0, "the rows' tables are aligned");
    static_assert(kCorWaveAt<K, E, NW> <= 2 * S * 2 * 64 * 16, "correct LDS fits the part buffers");
    const uint8_t* syn = ldsb + 1024;
    const PairGf& gf = *reinterpret_cast<const PairGf*>(ldsb + kCorGfAt<E>);
    CorRow* row = reinterpret_cast<CorRow*>(ldsb + kCorWaveAt<K, E, G>);
    uint8_t* wsyn = reinterpret_cast<uint8_t*>(row + K);
    unsigned done = 0;
    unsigned long long todo = __ballot(pend);
    while (todo) {
        const int c = c0 + __ffsll(todo) - 1;
        todo &= todo - 1;
        if (lane < E)
            wsyn[lane] = syn[lane * kSpanRow + c];
        const uint8_t s0 = syn[c], s1 = syn[kSpanRow + c], s2 = syn[2 * kSpanRow + c];
        for (int r = lane; r < K; r += 64)
            row[r] = rs_pair_row(gf, s0, s1, s2, r);
        // what a lane wrote is read by the other lanes of the wave from here on
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const CorPairs p = rs_pair_search_lane(gf, K, E, wsyn, row, lane);
        const long long lo = (long long)blockIdx.x * 2048 + (c >> 3) * 32;
        const bool one = __ballot(p.cnt >= 2) == 0 && __popcll(__ballot(p.cnt == 1)) == 1 && lo + 32 <= a.len;
        if (one && p.cnt == 1) {
            const long long at = lo + 8 * pass + (c & 7);
            uint8_t* ga = (p.ra < K ? a.src + ((size_t)wb * K + p.ra) * a.pitch
                                    : a.par + ((size_t)wb * E + (p.ra - K)) * a.pitch) + at;
            uint8_t* gb = (p.rb < K ? a.src + ((size_t)wb * K + p.rb) * a.pitch
                                    : a.par + ((size_t)wb * E + (p.rb - K)) * a.pitch) + at;
            *ga ^= p.xa;
            *gb ^= p.xb;
        }
        done += one;
        // the next column's syndromes overwrite what the lanes still read here
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    return done;
}

// Wave G's rows [R0, R0 + NR) of one tile.  The lane's 32 bytes of each
// stored parity row, as planes, XORed into the accumulators: the syndromes,
// in place.  Their OR over planes and rows gives the lane's bad-byte mask
// (idle lanes, which re-read the row head, give none); the NW waves' masks
// meet in LDS.  A clean tile ends there and writes nothing.  Otherwise wave
// 0 adds the tile's bad-column count to the block,
// and with `locate` the cold path names each bad column's row (rsgpu.h).  It
// is small code, not fast code: in four passes the waves lay 8 bytes per lane
// of all E syndrome rows into LDS (syn [E][512]), and the workgroup's threads
// walk the 512 columns byte by byte.  The code's ratios are c[1][j] / c[0][j]
// = 2^j, so the only source row that can explain (s_0, s_1) is r = log(s_1 /
// s_0), with x = s_0 (c[0][r] = 1), and it does when s_p == 2^(p r) x for
// every p; r >= K: no row; s_0 or s_1 zero: parity row k + p when s_p is the
// only non-zero syndrome.  The maxima of row + 1 and of kScrubBias - row go
// into the block's fold (order-independent atomics, one pair per wave).
// LDS, in the part buffers: masks [NW][64] u32 | syn = 1 + E / 2 KiB of the 32.
// The locate (A::kSpan) leaves here, after the count, for span_tile above.
//
// The repair (A::kRepair) corrects in that walk: the thread at column c of
// pass `pass` has the row and the error value x (s_0 for a source row, s_p0
// for parity row K + p0), and column c is byte 8 pass + c % 8 of lane c / 8's
// 32 bytes of the tile, so it XORs x into that byte of the global row: one
// byte read and written per bad column, in the cold path only.  In place is
// safe: by the barrier before the first pass every wave of the workgroup has
// read all it reads of the tile (the sources before run_group's last barrier,
// the stored parity before the mask barrier), and no other workgroup uses
// those bytes -- the idle lanes of a row's tail tile do re-read the row head,
// which the head's workgroup may be correcting, but what they read is
// discarded (`inb`).  An idle lane's syndromes are zeros, so none of its
// columns is bad; the lane bound is checked all the same before a write.
// kRepairLocate writes nothing, kRepairGated folds nothing (the block's
// report is final), kRepairColumns folds `row` over the corrected columns
// only and counts them, one atomic per wave.  The walk's repair part is one
// divergent region on purpose (address and value by selects, one `if` around
// the store, the fold by selects): every nesting level keeps a saved exec
// mask in an SGPR pair, and nested branches here cost the (64, 32) kernel 9
// SGPR spills in its main loop and 1 % of its time (profiles/repair).
//
// The correction (CorrectArgs) is the repair in its kRepairColumns mode on the
// 32-byte fold.  With t == 2 a bad column no row explains is pending: the wave
// takes a step's pending columns at the top of the next step
// (correct_pending, above), and folds its two-row corrections as `rep`, `two`
// and hi1 = lo1 = kScrubNoRow.  syn's rows then lie 520 bytes apart, as
// span_tile's, for the lanes that read a column's syndromes p = lane.
// Everything of it hangs off `kCorrect`; the other kernels' code is what it
// was (profiles/correct_fused).
template <int K, int E, int NW, int G, int R0, int NR, class A>
__device__ __forceinline__ void scrub_tile(const A& a, uint32_t (&acc)[NR][8], bool inb, long long wo,
                                           long long wb, long long blk, int lane, uint4* ldsv, uint32_t m4,
                                           uint32_t m2, uint32_t m1)
{
    static_assert(E >= 2 && 1024 + E * 512 <= 2 * S * 2 * 64 * 16, "scrub LDS fits the part buffers");
    constexpr bool kCorrect = std::is_same_v<A, CorrectArgs>;
    constexpr int kRow = kCorrect ? kSpanRow : 512;  // syn's row stride
    uint32_t* wmask = reinterpret_cast<uint32_t*>(ldsv);
    uint8_t* syn = reinterpret_cast<uint8_t*>(ldsv) + 1024;
    const uint8_t* pb = a.par + (size_t)wb * E * a.pitch;
    // The stored row goes to planes (one tr8, as the store epilogue spends on
    // the accumulators) and the syndromes stay planes: a byte is non-zero
    // when any of its 8 plane bits is, so the OR of a row's planes IS its
    // bad-byte mask (bit 8 q + w: byte 4 w + q), one register for all rows.
    // The stored row r + 1 is in flight while row r is transposed: one row
    // ahead, no further (the scheduler would otherwise hoist all NR rows'
    // loads, 8 VGPRs each, over the accumulators).
    // (An idle lane reads the row head, as it does of the sources: no branch
    // around the loads.)
    uint32_t mine = 0;
    uint32_t Pn[8];
    const long long po = inb ? wo : 0;
    load32(pb + (size_t)R0 * a.pitch, po, true, Pn);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        uint32_t Pw[8];
#pragma unroll
        for (int q = 0; q < 8; ++q)
            Pw[q] = Pn[q];
        if (r + 1 < NR)
            load32(pb + (size_t)(R0 + r + 1) * a.pitch, po, true, Pn);
        tr8(Pw, m4, m2, m1);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            acc[r][q] ^= Pw[q];
            mine |= acc[r][q];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    wmask[G * 64 + lane] = inb ? mine : 0u;
    __syncthreads();
    uint32_t tm = 0;
#pragma unroll
    for (int g = 0; g < NW; ++g)
        tm |= wmask[g * 64 + lane];
    if (__ballot(tm != 0) == 0)
        return;  // the same for every wave of the workgroup
    auto* f = a.fold + blk;
    if constexpr (G == 0) {
        unsigned n = __builtin_popcount(tm);
        for (int off = 32; off > 0; off >>= 1)
            n += __shfl_down(n, off, 64);
        bool count = lane == 0;
        if constexpr (A::kRepair)
            count = count && a.mode != kRepairGated;
        if (count)
            atomicAdd(&f->bad, (unsigned long long)n);
    }
    if constexpr (A::kSpan) {
        span_tile<E, NW, G, R0, NR>(a, acc, inb, tm, blk, lane, reinterpret_cast<uint8_t*>(ldsv), m4, m2, m1);
        return;
    }
    if (!a.locate)
        return;
    const uint8_t* gexp = kGfBs.exp;
    const uint8_t* glog = kGfBs.log;
    const int tid = G * 64 + lane;
    unsigned hi1 = 0, lo1 = 0;
    [[maybe_unused]] unsigned nrep = 0;
    [[maybe_unused]] unsigned ntwo = 0;  // the correction: the wave's columns corrected in two rows
    if constexpr (kCorrect)
        correct_tables<E, NW>(a, reinterpret_cast<uint8_t*>(ldsv), tid);  // read from the first pass's barrier on
#pragma unroll
    for (int rr = 0; rr < NR; ++rr)
        tr8(acc[rr], m4, m2, m1);  // syndrome planes -> bytes, in place
    for (int pass = 0; pass < 4; ++pass) {
        // the lane's bytes 8 pass .. 8 pass + 7 of every row (zeros from an idle lane)
        [&]<int... Ps>(std::integer_sequence<int, Ps...>) {
            ((pass == Ps ? [&] {
#pragma unroll
                for (int rr = 0; rr < NR; ++rr)
                    *reinterpret_cast<uint2*>(syn + (R0 + rr) * kRow + lane * 8) =
                        inb ? make_uint2(acc[rr][2 * Ps], acc[rr][2 * Ps + 1]) : make_uint2(0u, 0u);
            }()
                         : void()),
             ...);
        }(std::make_integer_sequence<int, 4>{});
        __syncthreads();
        // The correction: a step's pending column (bad, no row explains it)
        // goes to the wave when the step ends, by `continue` or not, while the
        // pass's syndromes are in LDS: the trip count is the same in every
        // lane, all 64 are there.
        [[maybe_unused]] bool pend = false;
        auto step_ends = [&]([[maybe_unused]] int c) {
            if constexpr (kCorrect) {
                if (a.t == 2)
                    ntwo += correct_pending<K, E, NW, G>(a, pend, c - lane, pass, wb, lane,
                                                         reinterpret_cast<uint8_t*>(ldsv));
                pend = false;
            }
        };
        for (int c = tid; c < 512; step_ends(c), c += 64 * NW) {
            const uint32_t s0 = syn[c], s1 = syn[kRow + c];
            int nz = 0, p0 = 0;
            for (int p = 0; p < E; ++p) {
                const bool on = syn[p * kRow + c] != 0;
                nz += on;
                p0 = on ? p : p0;
            }
            if (!nz)
                continue;
            int row = -1;
            if (s0 && s1) {
                int r = (int)glog[s1] + 255 - (int)glog[s0];  // c[1][r] / c[0][r] = 2^r
                r = r >= 255 ? r - 255 : r;
                if (r < K) {
                    const int lx = glog[s0];  // x = s_0: c[0][r] = 1
                    bool ok = true;
                    for (int p = 2; p < E; ++p)
                        ok &= syn[p * kRow + c] == gexp[(p * r) % 255 + lx];
                    row = ok ? r : -1;
                }
            } else if (nz == 1) {
                row = K + p0;
            }
            if constexpr (A::kRepair) {
                // the tile's byte offset of lane c / 8, and the column in it
                const long long lo = (long long)blockIdx.x * 2048 + (c >> 3) * 32;
                const bool src_row = row < K;
                uint8_t* g = (src_row ? a.src : a.par) +
                             ((size_t)wb * (src_row ? K : E) + (src_row ? row : row - K)) * a.pitch + lo +
                             8 * pass + (c & 7);
                const uint8_t x = src_row ? (uint8_t)s0 : syn[(row >= K ? row - K : 0) * kRow + c];
                if (a.mode != kRepairLocate && row >= 0 && lo + 32 <= a.len) {
                    *g ^= x;
                    ++nrep;
                }
                // what folds into `row`: every bad column (kRepairLocate), the
                // corrected ones (kRepairColumns), none (kRepairGated)
                const bool folds = a.mode == kRepairLocate || (a.mode == kRepairColumns && row >= 0);
                hi1 = max(hi1, !folds ? 0u : row >= 0 ? (unsigned)row + 1 : kScrubNoRow);
                lo1 = max(lo1, !folds ? 0u : row >= 0 ? kScrubBias - (unsigned)row : kScrubNoRow);
                if constexpr (kCorrect)
                    pend = row < 0;
                continue;
            }
            hi1 = max(hi1, row >= 0 ? (unsigned)row + 1 : kScrubNoRow);
            lo1 = max(lo1, row >= 0 ? kScrubBias - (unsigned)row : kScrubNoRow);
        }
        __syncthreads();  // the next pass overwrites syn
    }
    if constexpr (kCorrect) {
        // a two-row correction: no common row of the block's corrected columns
        hi1 = ntwo ? kScrubNoRow : hi1;
        lo1 = ntwo ? kScrubNoRow : lo1;
        nrep += lane == 0 ? ntwo : 0u;
        if (lane == 0 && ntwo)
            atomicAdd(&f->two, (unsigned long long)ntwo);
    }
    for (int off = 32; off > 0; off >>= 1) {
        hi1 = max(hi1, (unsigned)__shfl_down((int)hi1, off, 64));
        lo1 = max(lo1, (unsigned)__shfl_down((int)lo1, off, 64));
    }
    if (lane == 0 && hi1) {
        atomicMax(&f->hi1, hi1);
        atomicMax(&f->lo1, lo1);
    }
    if constexpr (A::kRepair) {
        for (int off = 32; off > 0; off >>= 1)
            nrep += __shfl_down(nrep, off, 64);
        if (lane == 0 && nrep && a.mode == kRepairColumns)
            atomicAdd(&f->rep, (unsigned long long)nrep);
    }
}

// The degraded scrub's epilogue (DegArgs): scrub_tile for a block with
// known-lost rows, on the tables k_degraded_prepare wrote for it (rs_kernels.h:
// the pivot parity rows Q, the other surviving parity rows `rest`, R and, with
// locate, every row's reduced column H).  One round trip fetches the header
// and the rest list (lane l: rest[l]), a second one, over the pivot barrier, R
// (lane l: the 8 factors of rest row l); what a parity row is -- pivot i, rest row pi, or lost -- is then a ballot
// per row of the wave, so every test below is wave-uniform.
//   syndromes  the stored row to planes and into the accumulators, as
//              scrub_tile; a lost parity row is not loaded and counts nowhere
//   pivots     the wave's pivot rows' planes go to slot i of the second part
//              buffer (a slot: [2][64] uint4 = 2 KB, at most 8), a barrier
//   reduction  t_p = s_p ^ XOR_i R[p][i] s_Q[i] for the wave's rest rows, the
//              pivot's planes read once per i and multiplied by the uniform
//              constant on planes (plane_mul.h); Q rows are zero by
//              construction, neither reduced nor counted
//   mask       the OR over the rest rows' planes; from there scrub_tile's
//              logic: masks meet in LDS, a clean tile leaves, wave 0 counts
// The cold path (a dirty tile with locate) lays t, as bytes, into LDS in four
// passes as scrub_tile lays its syndromes (the first pass may overwrite the
// pivot slots: every wave is past its reduction at the mask barrier), and the
// threads walk the 512 columns of a pass with deg_locate's rule (rs_degraded.hip)
// on the t bytes in LDS and H from the table: the first non-zero entry p*, a
// screen on one other entry, then t_p h_r[p*] == t_p* h_r[p] for every rest row;
// a row only when exactly one surviving row passes.  Small code, not fast code.
// LDS: masks 1 KiB | t [E][512] | rest [E]; the slots from 16 KiB on.
template <int K, int E, int NW, int G, int R0, int NR>
__device__ __forceinline__ void degraded_tile(const DegArgs& a, uint32_t (&acc)[NR][8], bool inb, long long wo,
                                              long long wb, long long blk, int lane, uint4* ldsv, uint32_t m4,
                                              uint32_t m2, uint32_t m1)
{
    static_assert(E >= 2 && E <= 64 && 1024 + E * 512 + E <= 2 * S * 2 * 64 * 16, "degraded LDS fits the part buffers");
    uint32_t* wmask = reinterpret_cast<uint32_t*>(ldsv);
    uint8_t* syn = reinterpret_cast<uint8_t*>(ldsv) + 1024;
    uint8_t* lrest = syn + E * 512;
    uint4* piv = ldsv + S * 2 * 64;
    const uint8_t* pb = a.par + (size_t)wb * E * a.pitch;
    const uint8_t* tab = a.tab + (size_t)blk * degraded_tab_stride(K, E);
    const uint8_t* t_rest = tab + sizeof(DegradedHdr);
    const uint8_t* t_r = t_rest + degraded_rest_bytes(E);
    // the block's table: every lane the header, lane l < E rest[l] and R[l]
    const uint4 hd = *reinterpret_cast<const uint4*>(tab);
    const int rv = lane < E ? t_rest[lane] : 0;
    const int nq = __builtin_amdgcn_readfirstlane((int)(hd.y & 0xFFu));
    const int nrest = __builtin_amdgcn_readfirstlane((int)((hd.y >> 8) & 0xFFu));
    const int qv = (int)(((lane & 4 ? hd.w : hd.z) >> (8 * (lane & 3))) & 0xFFu);  // lane i < 8: Q[i]
    const unsigned long long qlanes = (1ull << nq) - 1, rlanes = (1ull << nrest) - 1;  // nq <= 8, nrest <= E < 64
    int slot[NR], pi[NR];  // wave-uniform: the row's pivot slot / index among the rest rows, or -1
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const unsigned long long qm = __ballot(qv == R0 + r) & qlanes;
        const unsigned long long rm = __ballot(rv == R0 + r) & rlanes;
        slot[r] = qm ? __ffsll(qm) - 1 : -1;
        pi[r] = rm ? __ffsll(rm) - 1 : -1;
    }
    // the syndromes of the surviving parity rows, one stored row ahead as scrub_tile
    uint32_t Pn[8];
    const long long po = inb ? wo : 0;
    auto live = [&](int r) { return slot[r < NR ? r : 0] >= 0 || pi[r < NR ? r : 0] >= 0; };  // not a lost row
    load32(pb + (size_t)R0 * a.pitch, po, live(0), Pn);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        uint32_t Pw[8];
#pragma unroll
        for (int q = 0; q < 8; ++q)
            Pw[q] = Pn[q];
        if (r + 1 < NR)
            load32(pb + (size_t)(R0 + r + 1) * a.pitch, po, live(r + 1), Pn);
        if (live(r)) {
            tr8(Pw, m4, m2, m1);
#pragma unroll
            for (int q = 0; q < 8; ++q)
                acc[r][q] ^= Pw[q];
        }
        if (slot[r] >= 0) {
            piv[(slot[r] * 2 + 0) * 64 + lane] = make_uint4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
            piv[(slot[r] * 2 + 1) * 64 + lane] = make_uint4(acc[r][4], acc[r][5], acc[r][6], acc[r][7]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // R arrives over the barrier (loaded here, not with the header: two more
    // VGPRs across the loop above put (64, 32) into scratch)
    const uint2 rr8 = lane < E ? *reinterpret_cast<const uint2*>(t_r + lane * 8) : make_uint2(0u, 0u);
    __syncthreads();
    unsigned long long fac[NR];  // R[pi]: byte i the factor of pivot i
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int l = pi[r] >= 0 ? pi[r] : 0;
        fac[r] = (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)rr8.x, l) |
                 (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)rr8.y, l) << 32;
    }
    for (int i = 0; i < nq; ++i) {
        const uint4 u = piv[(i * 2 + 0) * 64 + lane], v = piv[(i * 2 + 1) * 64 + lane];
        const uint32_t sq[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const uint32_t c = (uint32_t)(fac[r] >> (8 * i)) & 0xFFu;
            if (pi[r] >= 0 && c)
                plane_mul_acc(acc[r], sq, c);
        }
    }
    uint32_t mine = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r)
        if (pi[r] >= 0) {
#pragma unroll
            for (int q = 0; q < 8; ++q)
                mine |= acc[r][q];
        }
    wmask[G * 64 + lane] = inb ? mine : 0u;
    __syncthreads();
    uint32_t tm = 0;
#pragma unroll
    for (int g = 0; g < NW; ++g)
        tm |= wmask[g * 64 + lane];
    if (__ballot(tm != 0) == 0)
        return;  // the same for every wave of the workgroup
    ScrubFold* f = a.fold + blk;
    if constexpr (G == 0) {
        unsigned n = __builtin_popcount(tm);
        for (int off = 32; off > 0; off >>= 1)
            n += __shfl_down(n, off, 64);
        if (lane == 0)
            atomicAdd(&f->bad, (unsigned long long)n);
    }
    if (!a.locate)
        return;
    const uint8_t* t_h = t_r + (size_t)E * 8;
    const int tid = G * 64 + lane;
    unsigned hi1 = 0, lo1 = 0;
    if (tid < nrest)
        lrest[tid] = t_rest[tid];  // read from the first pass's barrier on
#pragma unroll
    for (int r = 0; r < NR; ++r)
        tr8(acc[r], m4, m2, m1);  // planes -> bytes, in place (a Q or lost row: never read below)
    for (int pass = 0; pass < 4; ++pass) {
        // the lane's bytes 8 pass .. 8 pass + 7 of every row (zeros from an idle lane)
        [&]<int... Ps>(std::integer_sequence<int, Ps...>) {
            ((pass == Ps ? [&] {
#pragma unroll
                for (int r = 0; r < NR; ++r)
                    *reinterpret_cast<uint2*>(syn + (R0 + r) * 512 + lane * 8) =
                        inb ? make_uint2(acc[r][2 * Ps], acc[r][2 * Ps + 1]) : make_uint2(0u, 0u);
            }()
                         : void()),
             ...);
        }(std::make_integer_sequence<int, 4>{});
        __syncthreads();
        for (int c = tid; c < 512; c += 64 * NW) {
            int ps = -1;
            uint8_t ts = 0, t0 = 0, t2 = 0;
            for (int p = 0; p < nrest; ++p) {
                const uint8_t t = syn[lrest[p] * 512 + c];
                if (p == 0)
                    t0 = t;
                if (ps < 0 && t) {
                    ps = p;
                    ts = t;
                } else if (ps >= 0 && p == ps + 1) {
                    t2 = t;
                }
            }
            if (ps < 0)
                continue;  // not a bad column
            // the screen: entry 0 (zero) when p* > 0, else entry 1 when there is one
            const int p2 = ps > 0 ? 0 : nrest > 1 ? 1 : -1;
            if (ps > 0)
                t2 = t0;
            int found = 0, row = -1;
            for (int r = 0; r < K + E && found < 2; ++r) {
                const uint8_t* h = t_h + (size_t)r * E;
                const uint8_t hs = h[ps];
                if (!hs)
                    continue;
                if (p2 >= 0 && gf_mul_slow(t2, hs) != gf_mul_slow(ts, h[p2]))
                    continue;
                bool ok = true;
                for (int p = 0; p < nrest && ok; ++p)
                    ok = gf_mul_slow(syn[lrest[p] * 512 + c], hs) == gf_mul_slow(ts, h[p]);
                if (ok) {
                    ++found;
                    row = r;
                }
            }
            row = found == 1 ? row : -1;
            hi1 = max(hi1, row >= 0 ? (unsigned)row + 1 : kScrubNoRow);
            lo1 = max(lo1, row >= 0 ? kScrubBias - (unsigned)row : kScrubNoRow);
        }
        __syncthreads();  // the next pass overwrites t
    }
    for (int off = 32; off > 0; off >>= 1) {
        hi1 = max(hi1, (unsigned)__shfl_down((int)hi1, off, 64));
        lo1 = max(lo1, (unsigned)__shfl_down((int)lo1, off, 64));
    }
    if (lane == 0 && hi1) {
        atomicMax(&f->hi1, hi1);
        atomicMax(&f->lo1, lo1);
    }
}

// One wave group: rows [R0, R0+NR).  The workgroup streams the sources
// chunk by chunk (Horner order, last chunk first) through the LDS parts:
// while part n is transposed in place and consumed, part n+1 is already in
// flight by LDS-DMA (global_load_lds_dwordx4, counted vmcnt, raw barriers).
template <int K, int E, int C, int NW, int G, bool PRIO, class A = Args>
__device__ __forceinline__ void run_group(const A& a, uint4 (*lds)[S * 2 * 64])
{
    using P = PlanHolder<K, E, C>;
    constexpr int OPW = (E + NW - 1) / NW;
    constexpr int R0 = G * OPW;
    constexpr int NR = (E - R0) < OPW ? (E - R0) : OPW;
    constexpr int NCH = (K + C - 1) / C;
    constexpr int NP = (C + S - 1) / S;  // parts per chunk
    static_assert(NR > 0, "empty wave group");

    const int lane = threadIdx.x & 63;
    const TilePos tp = tile_pos(a, lane);
    const bool inb = tp.inb;
    // source offset from the tile's first block; out-of-range lanes re-read
    // the row head
    // (kernel_hooks.h: the diagnostic HBM-quiet variant moves both into a
    // two-block window)
    const long long wo = Hooks::data_offset(tp.o, blockIdx.x, lane);
    const long long wb = Hooks::data_block(tp.b0);
    const long long loff = inb ? tp.db * (long long)K * a.pitch + wo : 0;
    const uint8_t* sb = a.src + (size_t)wb * K * a.pitch;
    auto live = [&](int j) { return j < K; };
    const uint32_t m4 = vconst(0x0F0F0F0Fu), m2 = vconst(0x33333333u), m1 = vconst(0x55555555u);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4*)&lds[0][0];

    // step n -> (chunk, part): chunks in Horner order NCH-1 .. 0
    constexpr int NSTEP = NCH * NP;
    auto first_src = [&](int n) { return (NCH - 1 - n / NP) * C + (n % NP) * S; };
    auto part_len = [&](int n) {
        const int p = n % NP;
        return min(S, C - p * S);
    };
    // this wave's share of step n: t = G, G + NW, ...
    auto issue = [&](int n) {
        const int j0 = first_src(n), nt = part_len(n);
        const uint32_t base = lds0 + (uint32_t)((n & 1) * S * 2 * 64 * 16);
        for (int t = G; t < nt; t += NW)
            if (live(j0 + t))
                bs::glds32(sb + (size_t)(j0 + t) * a.pitch, (uint32_t)loff,
                           base + (uint32_t)(t * 2 * 64 * 16));
    };
    auto issued = [&](int n) {
        const int j0 = first_src(n), nt = part_len(n);
        int c = 0;
        for (int t = G; t < nt; t += NW)
            c += live(j0 + t) ? 2 : 0;
        return c;
    };

    uint32_t acc[NR][8];
    uint32_t p0[8] = {};  // planes of the current chunk's source 0 (T0Pair)
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int q = 0; q < 8; ++q)
            acc[r][q] = 0;

    issue(0);
    for (int n = 0; n < NSTEP; ++n) {
        uint4* buf = lds[n & 1];
        const int j0 = first_src(n), nt = part_len(n);
        if (n + 1 < NSTEP) {
            issue(n + 1);
            bs::wait_vm(issued(n + 1));
        } else {
            bs::wait_vm(0);
        }
        // the transposes up to the part barrier over the other workgroups'
        // multiply-accumulates (round 6, profiles/r06_prio/: encode -1.2 to -2.3 %)
        if constexpr (PRIO)
            asm volatile("s_setprio 2" ::: "memory");
        for (int t = G; t < nt; t += NW)
            if (live(j0 + t)) {
                uint4 u = buf[(t * 2 + 0) * 64 + lane];
                uint4 v = buf[(t * 2 + 1) * 64 + lane];
                uint32_t W[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
                if constexpr (!Hooks::kTransposes)
                    continue;
                tr8(W, m4, m2, m1);
                hook_planes<Hooks>(W);
                buf[(t * 2 + 0) * 64 + lane] = make_uint4(W[0], W[1], W[2], W[3]);
                buf[(t * 2 + 1) * 64 + lane] = make_uint4(W[4], W[5], W[6], W[7]);
            }
        bs::barrier_lds();
        if constexpr (PRIO)
            asm volatile("s_setprio 0" ::: "memory");
        const int part = n % NP;
        if (part == 0 && n != 0)
            twiddle_rows<P, R0, NR>(acc, std::make_integer_sequence<int, NR>{});
        // consume part `part` of the chunk: compile-time T = part*S + t
        [&]<int... Ps>(std::integer_sequence<int, Ps...>) {
            ((part == Ps ? consume_part<P, K, C, R0, NR, Ps>(acc, p0, buf, lane, j0)
                         : void()),
             ...);
        }(std::make_integer_sequence<int, NP>{});
        bs::barrier_lds();  // part buffer n & 1 is refilled by step n + 2
    }

    if constexpr (A::kScrub) {
        // the part buffers are free: every wave is past the last step's barrier
        if constexpr (A::kDegraded)
            degraded_tile<K, E, NW, G, R0, NR>(a, acc, inb, wo, wb, tp.b0, lane, &lds[0][0], m4, m2, m1);
        else
            scrub_tile<K, E, NW, G, R0, NR>(a, acc, inb, wo, wb, tp.b0, lane, &lds[0][0], m4, m2, m1);
    } else {
        if (!inb)
            return;
        uint8_t* ob = a.out + (size_t)wb * E * a.pitch;
        const long long ooff = tp.db * (long long)E * a.pitch + wo;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            uint32_t W[8];
#pragma unroll
            for (int q = 0; q < 8; ++q)
                W[q] = acc[r][q];
            tr8(W, m4, m2, m1);
            store32(ob + (size_t)(R0 + r) * a.pitch, ooff, W);
        }
    }
}

// waves per SIMD the register budget must allow: 4 while a wave owns <= 8 rows
// (64 accumulator VGPRs), 2 for 16 rows (128 accumulators; halves the
// per-wave four-Russians table builds, but measured slower at (64, 32):
// 24.2 vs 23.2 ms, two waves per SIMD do not hide the LDS-DMA pipeline)
template <int E, int NW>
constexpr int bs_waves_per_simd()
{
    return (E + NW - 1) / NW > 8 ? 2 : 16 / NW;
}

template <int K, int E, int C, int NW, bool PRIO = true>
__global__ __launch_bounds__(64 * NW, (bs_waves_per_simd<E, NW>())) void k_rs_bs(Args a)
{
    __shared__ uint4 lds[2][S * 2 * 64];
    RSGPU_DIAG_BEGIN()
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    [&]<int... Gs>(std::integer_sequence<int, Gs...>) {
        ((wave == Gs ? run_group<K, E, C, NW, Gs, PRIO>(a, lds) : void()), ...);
    }(std::make_integer_sequence<int, NW>{});
    RSGPU_DIAG_END();
}

// The scrub: k_rs_bs's accumulation (wave priority window on) with
// scrub_tile as the epilogue.
template <int K, int E, int C, int NW>
__global__ __launch_bounds__(64 * NW, (bs_waves_per_simd<E, NW>())) void k_rs_bs_scrub(ScrubArgs a)
{
    __shared__ uint4 lds[2][S * 2 * 64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    [&]<int... Gs>(std::integer_sequence<int, Gs...>) {
        ((wave == Gs ? run_group<K, E, C, NW, Gs, true, ScrubArgs>(a, lds) : void()), ...);
    }(std::make_integer_sequence<int, NW>{});
}

// The locate: k_rs_bs_scrub with span_tile as the cold path of the epilogue.
template <int K, int E, int C, int NW>
__global__ __launch_bounds__(64 * NW, (bs_waves_per_simd<E, NW>())) void k_rs_bs_locate(LocArgs a)
{
    __shared__ uint4 lds[2][S * 2 * 64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    [&]<int... Gs>(std::integer_sequence<int, Gs...>) {
        ((wave == Gs ? run_group<K, E, C, NW, Gs, true, LocArgs>(a, lds) : void()), ...);
    }(std::make_integer_sequence<int, NW>{});
}

// The repair: k_rs_bs_scrub with the correcting epilogue.  kRepairGated runs
// after the finalise of a kRepairLocate pass on the same stream: the block's
// verdict is read (a scalar load, the block index is uniform) and a workgroup
// whose block is not to be written leaves before it loads anything.
template <int K, int E, int C, int NW>
__global__ __launch_bounds__(64 * NW, (bs_waves_per_simd<E, NW>())) void k_rs_bs_repair(RepairArgs a)
{
    __shared__ uint4 lds[2][S * 2 * 64];
    if (a.mode == kRepairGated && a.fold[blockIdx.y].hi1 != kRepairGate)
        return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    [&]<int... Gs>(std::integer_sequence<int, Gs...>) {
        ((wave == Gs ? run_group<K, E, C, NW, Gs, true, RepairArgs>(a, lds) : void()), ...);
    }(std::make_integer_sequence<int, NW>{});
}

// The correction per column: k_rs_bs_repair in its kRepairColumns mode whose
// walk, with t == 2, takes the columns no row explains to correct_pending.
template <int K, int E, int C, int NW>
__global__ __launch_bounds__(64 * NW, (bs_waves_per_simd<E, NW>())) void k_rs_bs_correct(CorrectArgs a)
{
    __shared__ uint4 lds[2][S * 2 * 64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    [&]<int... Gs>(std::integer_sequence<int, Gs...>) {
        ((wave == Gs ? run_group<K, E, C, NW, Gs, true, CorrectArgs>(a, lds) : void()), ...);
    }(std::make_integer_sequence<int, NW>{});
}

// The degraded scrub: k_rs_bs_scrub with degraded_tile as the epilogue.  A
// workgroup whose block the prepare has already reported (state != kDegRun:
// a malformed list, n == e, a matrix that does not determine D) leaves before
// it loads anything; the block index is uniform, the state a scalar load.
template <int K, int E, int C, int NW>
__global__ __launch_bounds__(64 * NW, (bs_waves_per_simd<E, NW>())) void k_rs_bs_degraded(DegArgs a)
{
    __shared__ uint4 lds[2][S * 2 * 64];
    if (reinterpret_cast<const DegradedHdr*>(a.tab + (size_t)blockIdx.y * degraded_tab_stride(K, E))->state != kDegRun)
        return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the first match ends the chain: with the siblings' `? :` fold hipcc keeps
    // the lane and the tile offsets alive through the group that runs, for the
    // groups after it, at (64, 32) and (100, 20) in scratch
    [&]<int... Gs>(std::integer_sequence<int, Gs...>) {
        (void)((wave == Gs && (run_group<K, E, C, NW, Gs, true, DegArgs>(a, lds), true)) || ...);
    }(std::make_integer_sequence<int, NW>{});
}

// Small batches of a single-chunk code (C == K, E <= 8; C2: one block of
// (16, 4, 1e6), 489 tiles, where one wave per tile leaves most SIMDs idle
// and walks all K sources in series): SPL waves split a tile's sources,
// wave w taking T = w, w + SPL, ... with the compile-time programs of those
// T (no source 0 pairing: the partner may belong to another wave), straight
// from global memory into registers; the partial accumulators meet in LDS
// and wave w finishes rows w, w + SPL, ...
template <int K, int E, int SPL, int G>
__device__ __forceinline__ void split_group(const Args& a, uint32_t (&acc)[E][8], long long loff)
{
    using P = PlanHolder<K, E, K>;
    const uint8_t* sb = a.src + (size_t)blockIdx.y * K * a.pitch;
    constexpr int NT = (K - G + SPL - 1) / SPL;  // this wave's sources
    uint32_t W[NT][8];
#pragma unroll
    for (int i = 0; i < NT; ++i)  // every load in flight before the first use
        load32(sb + (size_t)(G + SPL * i) * a.pitch, loff, true, W[i]);
    const uint32_t m4 = vconst(0x0F0F0F0Fu), m2 = vconst(0x33333333u), m1 = vconst(0x55555555u);
    const uint32_t none[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    [&]<int... Is>(std::integer_sequence<int, Is...>) {
        (
            [&] {
                tr8(W[Is], m4, m2, m1);
                consume<P, 0, E, G + SPL * Is, false>(acc, W[Is], none);
            }(),
            ...);
    }(std::make_integer_sequence<int, NT>{});
}

template <int K, int E, int SPL>
__global__ __launch_bounds__(64 * SPL) void k_rs_bs_split(Args a)
{
    static_assert(E <= 8 && K >= SPL, "split encode: one row group, every wave a source");
    __shared__ uint32_t part[SPL][E * 8][64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long long off = (long long)blockIdx.x * 2048 + lane * 32;
    const bool inb = off + 32 <= a.len;
    const long long loff = inb ? off : 0;  // out-of-range lanes re-read the row head
    uint32_t acc[E][8];
#pragma unroll
    for (int r = 0; r < E; ++r)
#pragma unroll
        for (int q = 0; q < 8; ++q)
            acc[r][q] = 0;
    [&]<int... Gs>(std::integer_sequence<int, Gs...>) {
        ((wave == Gs ? split_group<K, E, SPL, Gs>(a, acc, loff) : void()), ...);
    }(std::make_integer_sequence<int, SPL>{});
#pragma unroll
    for (int r = 0; r < E; ++r)
#pragma unroll
        for (int q = 0; q < 8; ++q)
            part[wave][r * 8 + q][lane] = acc[r][q];
    __syncthreads();
    if (!inb)
        return;
    const uint32_t m4 = vconst(0x0F0F0F0Fu), m2 = vconst(0x33333333u), m1 = vconst(0x55555555u);
    uint8_t* ob = a.out + (size_t)blockIdx.y * E * a.pitch;
    for (int r = wave; r < E; r += SPL) {
        uint32_t W[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int w = 0; w < SPL; ++w)
#pragma unroll
            for (int q = 0; q < 8; ++q)
                W[q] ^= part[w][r * 8 + q][lane];
        tr8(W, m4, m2, m1);
        store32(ob + (size_t)r * a.pitch, off, W);
    }
}

template <int K, int E>
hipError_t launch_split(const uint8_t* src, uint8_t* out, long long pitch, long long len, long long blocks,
                        hipStream_t st)
{
    Args a{src, out, pitch, len, blocks, 0};
    dim3 grid((unsigned)((len + 2047) / 2048), (unsigned)blocks);
    hipLaunchKernelGGL((k_rs_bs_split<K, E, 4>), grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Small decode batches of a single-chunk compiled code (C2: one block of
// (16, 4, 1e6)): syndromes through the encode's compile-time programs, then
// the e x e solve with runtime coefficients, in ONE launch.
//
// isa.cpp:169-213 applies rows of inv(b); the erased originals E also solve
// d_E = V_E^-1 s with s = P ^ V_Ebar d_Ebar (the same unique
// bytes).  V_Ebar holds the code's own entries 2^(p j), so each surviving
// original goes through consume<> exactly as in the encode (a uniform branch
// skips an erased one) and the parity rows are XORed in: no closed form and
// no threaded code for the e x k part.  Row i of V_E^-1 is [z^p] Q_i(z) / w_i,
// Q_i = prod_{l != i} (z + a_l), a_l = 2^(j_l), w_i = Q_i(a_i), built
// lane-parallel while the sources fly (lane 8 i + m: [z^m] Q_i, as
// k_rs_tc_fused builds its parity coefficients).  A runtime coefficient c
// applies through its 8 x 8 bit matrix: plane b of c x is the XOR over a of
// plane a of x where bit b of c 2^a is set, one v_bitop3 (out ^ (s & mask),
// mask an SGPR of 0 or ~0) per (a, b).  Four waves per 2 KB tile split the
// sources as k_rs_bs_split; the partial syndromes meet in LDS, each wave
// XORing its partials into one zeroed copy (ds_xor_b32), so the output phase
// reads every syndrome once instead of once per wave: C2 698-701 vs 687-689
// GiB/s, same box x4 (profiles/r04_spl/ldsx_*).  (The tables: kGfBs, above.)

// parity rows p = G, G + SPL, ... of wave G: they survive whatever the
// erasure list says, so their loads go out before the list arrives
template <int E, int SPL, int G>
__device__ __forceinline__ void syn_parity_loads(const SynArgs& a, long long loff, uint32_t (&Pw)[2][8])
{
    constexpr int NP = (E - G + SPL - 1) / SPL;
    static_assert(NP <= 2, "two parity rows per wave at most");
#pragma unroll
    for (int i = 0; i < NP; ++i)
        load32(a.par + ((size_t)blockIdx.y * E + G + SPL * i) * a.pitch, loff, true, Pw[i]);
}

template <class F, int K, int E, int SPL, int G>
__device__ __forceinline__ void syn_group(const SynArgs& a, unsigned long long emask, long long loff,
                                          uint32_t (&acc)[E][8], uint32_t (&Pw)[2][8], F&& between)
{
    using P = PlanHolder<K, E, K>;
    const int b = blockIdx.y;
    const uint8_t* sb = a.src + (size_t)b * K * a.pitch;
    constexpr int NT = (K - G + SPL - 1) / SPL;  // this wave's sources T = G, G + SPL, ...
    constexpr int NP = (E - G + SPL - 1) / SPL;  // its parity rows p = G, G + SPL, ...
    uint32_t W[NT][8];
    // every source load in flight at once; an erased original is never read
#pragma unroll
    for (int i = 0; i < NT; ++i)
        load32(sb + (size_t)(G + SPL * i) * a.pitch, loff, !((emask >> (G + SPL * i)) & 1), W[i]);
    between();  // the solve's coefficients, while the loads fly
    const uint32_t m4 = vconst(0x0F0F0F0Fu), m2 = vconst(0x33333333u), m1 = vconst(0x55555555u);
    const uint32_t none[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    [&]<int... Is>(std::integer_sequence<int, Is...>) {
        (
            [&] {
                constexpr int T = G + SPL * Is;
                if (!((emask >> T) & 1)) {
                    tr8(W[Is], m4, m2, m1);
                    consume<P, 0, E, T, false>(acc, W[Is], none);
                }
            }(),
            ...);
    }(std::make_integer_sequence<int, NT>{});
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        tr8(Pw[i], m4, m2, m1);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            acc[G + SPL * i][q] ^= Pw[i][q];
    }
}

template <int K, int E, int SPL>
__global__ __launch_bounds__(64 * SPL) void k_rs_syn_split(SynArgs a)
{
    static_assert(E <= 8 && K <= 64 && K >= SPL, "one chunk, e <= 8");
    __shared__ uint32_t syn[E * 8][64];  // the syndromes: every wave's partials XORed in
    __shared__ uint32_t gtw[SPL][192];  // per wave: exp[512] | log[256]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.y;
    const long long off = (long long)blockIdx.x * 2048 + lane * 32;
    const bool inb = off + 32 <= a.len;
    const long long loff = inb ? off : 0;  // out-of-range lanes re-read the row head
    uint32_t Pw[2][8];
    [&]<int... Gs>(std::integer_sequence<int, Gs...>) {
        ((wave == Gs ? syn_parity_loads<E, SPL, Gs>(a, loff, Pw) : void()), ...);
    }(std::make_integer_sequence<int, SPL>{});
    for (int i = threadIdx.x; i < E * 8 * 64; i += 64 * SPL)
        (&syn[0][0])[i] = 0;
    __syncthreads();
    // the GF tables and the block's erasure list in one round trip
    const uint32_t* tsrc = reinterpret_cast<const uint32_t*>(&kGfBs);
    const uint32_t t0 = tsrc[lane], t1 = tsrc[64 + lane], t2 = tsrc[128 + lane];
    // lane i: erased original j_i.  The block's list through the scalar
    // cache: the aligned words holding its E bytes (never past the word that
    // holds the last one); C2 678-680 vs 674-676 GiB/s with a vector load,
    // same box x4 (profiles/r04_slist/)
    int j;
    {
        typedef const uint32_t __attribute__((address_space(4)))* CW;
        const uint8_t* lp = a.err + (size_t)b * E;  // any alignment (a slice's list)
        const size_t off = (uintptr_t)lp & 3;
        const CW wp = (CW)(lp - off);
        constexpr int NW = (3 + E + 3) / 4;
        uint32_t w[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i)
            w[i] = (off + E + 3) / 4 > (size_t)i ? wp[i] : 0u;
        const int p = (int)off + lane;  // this lane's byte
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i)
            v = (p >> 2) == i ? w[i] : v;
        j = lane < E ? (int)((v >> (8 * (p & 3))) & 0xFFu) : 255;
    }
    const int jp = __shfl_up(j, 1);
    if (__ballot(lane < E && (j >= K || (lane > 0 && j <= jp))) != 0) {  // strictly ascending, < k
        if (blockIdx.x == 0 && threadIdx.x == 0)
            a.status[b] = -2;
        return;  // uniform per workgroup
    }
    bool er = false;
#pragma unroll
    for (int i = 0; i < E; ++i)
        er |= __builtin_amdgcn_readlane(j, i) == lane;
    const unsigned long long emask = __ballot(lane < K && er);
    uint32_t* gw = gtw[wave];
    gw[lane] = t0;
    gw[64 + lane] = t1;
    gw[128 + lane] = t2;
    const uint8_t* gexp = reinterpret_cast<const uint8_t*>(gw);
    const uint8_t* glog = gexp + 512;
    int coef = 0;  // lane 8 i + m: (V_E^-1)[i][m]
    auto solve_rows = [&] {
        const int i = lane >> 3, m = lane & 7;
        int J[8], A[8];
#pragma unroll
        for (int l = 0; l < 8; ++l)
            J[l] = __builtin_amdgcn_readlane(j, l);
        const int al = lane < E ? gexp[j] : 0;
#pragma unroll
        for (int l = 0; l < 8; ++l)
            A[l] = __builtin_amdgcn_readlane(al, l);
        int ji = 0, ai = 0;
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            ji = i == l ? J[l] : ji;
            ai = i == l ? A[l] : ai;
        }
        const int tv = gexp[(ji + m) % 255];  // lane 8 l + c: a_l 2^c = 2^(j_l + c)
        int qv = m == 0;                      // Q_i, one factor (z + a_l) at a time
#pragma unroll
        for (int l = 0; l < E; ++l) {
            int pr = 0;  // a_l q_m from the 2^c multiples of a_l where q_m has bit c
#pragma unroll
            for (int c = 0; c < 8; ++c)
                pr ^= __builtin_amdgcn_readlane(tv, l * 8 + c) & -((qv >> c) & 1);
            int sh = __builtin_amdgcn_update_dpp(0, qv, 0x111, 0xF, 0xF, true);  // row_shr:1, q_{m-1}
            sh = m ? sh : 0;
            qv = l == i ? qv : (sh ^ pr);
        }
        int lw = 0;  // log w_i = sum_{l != i} log (a_i + a_l)
#pragma unroll
        for (int l = 0; l < E; ++l)
            lw += glog[l != i ? (ai ^ A[l]) : 1];
        coef = (i < E && m < E && qv) ? gexp[(glog[qv] + 255 * 2 - lw % 255) % 255] : 0;
    };
    uint32_t acc[E][8];
#pragma unroll
    for (int r = 0; r < E; ++r)
#pragma unroll
        for (int q = 0; q < 8; ++q)
            acc[r][q] = 0;
    [&]<int... Gs>(std::integer_sequence<int, Gs...>) {
        ((wave == Gs ? syn_group<decltype(solve_rows)&, K, E, SPL, Gs>(a, emask, loff, acc, Pw, solve_rows) : void()),
         ...);
    }(std::make_integer_sequence<int, SPL>{});
    if (blockIdx.x == 0 && threadIdx.x == 0)
        a.status[b] = 0;
#pragma unroll
    for (int r = 0; r < E; ++r)
#pragma unroll
        for (int q = 0; q < 8; ++q)
            atomicXor(&syn[r * 8 + q][lane], acc[r][q]);  // ds_xor_b32, no return
    __syncthreads();
    if (!inb)
        return;
    // wave w's output rows r = w, w + SPL, ...: out_r = sum_p c[r][p] s_p,
    // each syndrome s_p already the sum of the waves' partials
    const uint32_t m4 = vconst(0x0F0F0F0Fu), m2 = vconst(0x33333333u), m1 = vconst(0x55555555u);
    for (int r = wave; r < E; r += SPL) {
        uint32_t o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int p = 0; p < E; ++p) {
            uint32_t sy[8];
#pragma unroll
            for (int q = 0; q < 8; ++q)
                sy[q] = syn[p * 8 + q][lane];
            uint32_t x = (uint32_t)__builtin_amdgcn_readlane(coef, 8 * r + p);  // c, then c 2^a
#pragma unroll
            for (int ab = 0; ab < 8; ++ab) {
#pragma unroll
                for (int bb = 0; bb < 8; ++bb)
                    o[bb] = __builtin_amdgcn_bitop3_b32(o[bb], sy[ab], 0u - ((x >> bb) & 1u), 0x78);
                x = ((x << 1) ^ ((x & 0x80u) ? 0x1Du : 0u)) & 0xFFu;
            }
        }
        tr8(o, m4, m2, m1);
        store32(a.out + ((size_t)b * E + r) * a.pitch, off, o);
    }
}

template <int K, int E>
hipError_t launch_syn(const SynArgs& a, long long blocks, hipStream_t st)
{
    dim3 grid((unsigned)((a.len + 2047) / 2048), (unsigned)blocks);
    hipLaunchKernelGGL((k_rs_syn_split<K, E, 4>), grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

template <int K, int E, int C, int NW>
hipError_t launch(const uint8_t* src, uint8_t* out, long long pitch, long long len,
                  long long blocks, hipStream_t st, int prio)
{
    // short rows whose last tile is partial: tiles over the rows of all
    // blocks end to end (tile_pos).  A lane addresses its rows from the
    // tile's first block with a 32-bit offset (glds32's voffset): db * K *
    // pitch + o, db <= 2048 / len + 1, must stay below 2^32
    const bool flat = blocks > 1 && len % 2048 != 0 && len < 65536 && pitch % 32 == 0 &&
                      (unsigned long long)(2048 / len + 2) * K * (unsigned long long)pitch < (1ull << 32);
    Args a{src, out, pitch, len, blocks, flat ? 1 : 0, prio};
    dim3 grid(flat ? (unsigned)((blocks * len + 2047) / 2048) : (unsigned)((len + 2047) / 2048),
              flat ? 1u : (unsigned)blocks);
    if (prio)
        hipLaunchKernelGGL((k_rs_bs<K, E, C, NW, true>), grid, dim3(64 * NW), 0, st, a);
    else
        hipLaunchKernelGGL((k_rs_bs<K, E, C, NW, false>), grid, dim3(64 * NW), 0, st, a);
    return hipGetLastError();
}

RSGPU_DIAG_READER(diag_read_bs)

// One compiled code (RSGPU_BS_PLANS, enc_progs.inc) as a type.  kSplit: the
// codes of the split kernels (k_rs_bs_split, k_rs_syn_split), a single chunk
// and one row group.
template <int K_, int E_, int C_, int NW_>
struct Plan {
    static constexpr int K = K_, E = E_, C = C_, NW = NW_;
    static constexpr bool kSplit = C == K && E <= 8;
};

// the split subset is (16, 4), (16, 8), (5, 4) and (20, 7), no more and no less
#define X(K, E, C, NW) \
    static_assert(Plan<K, E, C, NW>::kSplit == ((K == 16 && (E == 4 || E == 8)) || (K == 5 && E == 4) || (K == 20 && E == 7)));
RSGPU_BS_PLANS(X)
#undef X
#define X(K, E, C, NW) +Plan<K, E, C, NW>::kSplit
static_assert(0 RSGPU_BS_PLANS(X) == 4);
#undef X

// The one dispatch from a call's (k, e) to its compile-time plan:
// f(Plan<K, E, C, NW>{}), or `none` for a code that is not compiled.
template <class R, class F>
R with_plan(int k, int e, R none, F&& f)
{
#define X(K, E, C, NW) \
    if (k == K && e == E) \
        return f(Plan<K, E, C, NW>{});
    RSGPU_BS_PLANS(X)
#undef X
    return none;
}

// what the scrub, the locate, the degraded scrub and the repair ask of their rows
bool family_rows(long long blocks, long long len, long long pitch, const void* src, const void* par, const void* fold)
{
    return blocks > 0 && blocks <= 65535 && len > 0 && len % 32 == 0 && len < (1ll << 32) && pitch >= len && src &&
           par && fold;
}

// One launch of the plan's kernel of a scrub-family form, kernel_of(plan), on
// that form's Args: a workgroup of NW waves per tile and block.
template <class A, class KernelOf>
hipError_t launch_family(int k, int e, const A& a, hipStream_t st, KernelOf&& kernel_of)
{
    return with_plan(k, e, hipErrorInvalidValue, [&](auto p) {
        dim3 grid((unsigned)((a.len + 2047) / 2048), (unsigned)a.blocks);
        hipLaunchKernelGGL(kernel_of(p), grid, dim3(64 * p.NW), 0, st, a);
        return hipGetLastError();
    });
}

}  // namespace bs

bool rs_bitsliced_available(int k, int e)
{
    return bs::with_plan(k, e, false, [](auto) { return true; });
}

int rs_bitsliced_rows_per_wave(int k, int e)
{
    return bs::with_plan(k, e, 0, [](auto p) { return (p.E + p.NW - 1) / p.NW; });
}

bool rs_bitsliced_split_available(int k, int e)
{
    return bs::with_plan(k, e, false, [](auto p) { return p.kSplit; });
}

hipError_t launch_rs_bitsliced_split(int k, int e, const uint8_t* src, uint8_t* out, long long pitch,
                                     long long len, long long blocks, hipStream_t st)
{
    return bs::with_plan(k, e, hipErrorInvalidValue, [&](auto p) {
        if constexpr (p.kSplit)
            return bs::launch_split<p.K, p.E>(src, out, pitch, len, blocks, st);
        else
            return hipErrorInvalidValue;
    });
}

hipError_t launch_rs_syn_split(int k, int e, const SynArgs& a, long long blocks, hipStream_t st)
{
    if (blocks <= 0 || blocks > 65535 || a.len <= 0 || a.len % 32 != 0 || !a.src || !a.par || !a.out || !a.err ||
        !a.status)
        return hipErrorInvalidValue;
    return bs::with_plan(k, e, hipErrorInvalidValue, [&](auto p) {
        if constexpr (p.kSplit)
            return bs::launch_syn<p.K, p.E>(a, blocks, st);
        else
            return hipErrorInvalidValue;
    });
}

hipError_t launch_rs_bitsliced(int k, int e, const uint8_t* src, uint8_t* out, long long pitch,
                               long long len, long long blocks, hipStream_t st, int prio)
{
    return bs::with_plan(k, e, hipErrorInvalidValue, [&](auto p) {
        return bs::launch<p.K, p.E, p.C, p.NW>(src, out, pitch, len, blocks, st, prio);
    });
}

hipError_t launch_rs_bitsliced_scrub(int k, int e, const uint8_t* src, const uint8_t* par, long long pitch,
                                     long long len, long long blocks, ScrubFold* fold, int locate,
                                     hipStream_t st)
{
    if (!bs::family_rows(blocks, len, pitch, src, par, fold))
        return hipErrorInvalidValue;
    const bs::ScrubArgs a{src, par, pitch, len, blocks, fold, locate};
    return bs::launch_family(k, e, a, st, [](auto p) { return bs::k_rs_bs_scrub<p.K, p.E, p.C, p.NW>; });
}

hipError_t launch_rs_bitsliced_locate(int k, int e, const uint8_t* src, const uint8_t* par, long long pitch,
                                      long long len, long long blocks, ScrubFold* fold, uint8_t* cand,
                                      size_t cand_stride, int u, hipStream_t st)
{
    if (!bs::family_rows(blocks, len, pitch, src, par, fold) || !cand || u < 1 || u > kLocMax ||
        cand_stride < (size_t)((len + 2047) / 2048) * kLocateSlotBytes)
        return hipErrorInvalidValue;
    const bs::LocArgs a{src, par, pitch, len, blocks, fold, cand, cand_stride, u};
    return bs::launch_family(k, e, a, st, [](auto p) { return bs::k_rs_bs_locate<p.K, p.E, p.C, p.NW>; });
}

hipError_t launch_rs_bitsliced_degraded(int k, int e, const uint8_t* src, const uint8_t* par, long long pitch,
                                        long long len, long long blocks, const uint8_t* tab, ScrubFold* fold,
                                        int locate, hipStream_t st)
{
    if (!bs::family_rows(blocks, len, pitch, src, par, fold) || !tab || (uintptr_t)tab % 16 != 0)
        return hipErrorInvalidValue;
    const bs::DegArgs a{src, par, pitch, len, blocks, tab, fold, locate};
    return bs::launch_family(k, e, a, st, [](auto p) { return bs::k_rs_bs_degraded<p.K, p.E, p.C, p.NW>; });
}

hipError_t launch_rs_bitsliced_repair(int k, int e, uint8_t* src, uint8_t* par, long long pitch, long long len,
                                      long long blocks, RepairFold* fold, int mode, hipStream_t st)
{
    if (!bs::family_rows(blocks, len, pitch, src, par, fold) || mode < kRepairLocate || mode > kRepairColumns)
        return hipErrorInvalidValue;
    const bs::RepairArgs a{src, par, pitch, len, blocks, fold, mode};
    return bs::launch_family(k, e, a, st, [](auto p) { return bs::k_rs_bs_repair<p.K, p.E, p.C, p.NW>; });
}

hipError_t launch_rs_bitsliced_correct(int k, int e, uint8_t* src, uint8_t* par, long long pitch, long long len,
                                       long long blocks, CorrectFold* fold, int t, hipStream_t st)
{
    if (!bs::family_rows(blocks, len, pitch, src, par, fold) || !((t == 1 && e >= 3) || (t == 2 && e >= 5 && e <= 64)))
        return hipErrorInvalidValue;
    const bs::CorrectArgs a{src, par, pitch, len, blocks, fold, t};
    return bs::launch_family(k, e, a, st, [](auto p) { return bs::k_rs_bs_correct<p.K, p.E, p.C, p.NW>; });
}

}  // namespace rsgpu
