// rsgpu_internal.h -- host helpers that rsgpu_capi.cpp defines and the other
// host files of librsgpu share (rsgpu_decode.cpp, rsgpu_scrub.cpp), and the
// small rules all three follow.  Internal: rsgpu.map keeps all of it out of
// the library's exports.
#pragma once
#include <algorithm>
#include <vector>

#include "gf256.h"
#include "rs_kernels.h"
#include "rsgpu_ctx.h"

namespace rsgpu {

// column tiles of a row: what one workgroup of the row kernels covers
constexpr size_t kTileBytes = 2048;
inline size_t tiles(size_t len) { return (len + kTileBytes - 1) / kTileBytes; }

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// rows the kernels may read and write as 16-byte vectors
inline bool ptrs_aligned(size_t pitch, const void* a, const void* b, const void* c = nullptr)
{
    return pitch % 16 == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0 && (uintptr_t)c % 16 == 0;
}
// ... of a length the threaded and the generated code take
inline bool rows_aligned(size_t len, size_t pitch, const void* a, const void* b, const void* c = nullptr)
{
    return len % 32 == 0 && ptrs_aligned(pitch, a, b, c);
}

// The block index is grid.y: f(b0, nb) over consecutive slices of at most
// kMaxGridBlocks blocks, in stream order, up to the first error.
template <class F>
int for_grid_slices(size_t blocks, F&& f)
{
    for (size_t b0 = 0; b0 < blocks; b0 += kMaxGridBlocks)
        if (const int rc = f(b0, std::min(kMaxGridBlocks, blocks - b0)))
            return rc;
    return RSGPU_OK;
}

// the e x k parity matrix of a call: `coef`, or the gf_gen_rs_matrix rows
std::vector<uint8_t> parity_matrix(int k, int e, const unsigned char* coef);

const GfTables& host_gf();
uint8_t hmul(uint8_t a, uint8_t b);

// the argument check every block-batched entry point starts with
int check_geom(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks);

// rsgpu_ec_encode_data_batch's argument check behind the context (the test
// hooks run it without a device): tables stands for gftbls, d_data, d_coding
// and d_len all given
inline bool ec_batch_args_ok(int k, int rows, bool tables, int max_len, int flags)
{
    return k > 0 && k <= RSGPU_MAX_SOURCES && rows >= 0 && rows <= 255 && max_len >= 0 &&
           (flags & ~RSGPU_BATCH_ALIGNED32) == 0 && (rows == 0 || tables);
}

// Grow b to >= bytes (a fresh allocation of at least `floor`), its key
// cleared.  Every kernel that may still read the old buffer was enqueued on
// the context stream, or on an earlier stream the current one waits on
// (rsgpu_set_stream), so synchronising the current stream retires them all
// before the free.
int ensure_device(rsgpu_ctx* ctx, rsgpu_ctx::DevBuf& b, size_t bytes, size_t floor = 0);

// A pinned staging pointer of >= bytes, after the previous upload from it has
// completed; upload() sends `bytes` from stage_off of it to d_dst + dst_off.
int get_stage(rsgpu_ctx* ctx, size_t bytes, void** out);
int upload(rsgpu_ctx* ctx, void* d_dst, size_t bytes, size_t dst_off = 0, size_t stage_off = 0);

hipEvent_t pool_event(rsgpu_ctx* ctx);

// a timing-disabled event for cross-stream ordering, recycled round-robin
hipEvent_t sync_event(rsgpu_ctx* ctx);

// the handler table of k_rs_tc (rs_tc.hip) is located and ctx->d_tc_table holds
// its addresses; probed once per context
bool tc_handlers_ready(rsgpu_ctx* ctx);

// the device has a pool for executable allocations (1), or not (-1); probed
// once per context
int jit_probe(rsgpu_ctx* ctx);

// The row-pointer tables [blocks][k] of d_src and [blocks][e] of d_par (rows
// `pitch` bytes apart) at the head of the context's scratch, which is grown to
// hold them and `extra` bytes behind them (from `bytes` on) before the two
// launches that fill them are enqueued.
struct RowPtrs {
    const uint8_t* const* src;
    uint8_t* const* par;
    size_t bytes;
};
int row_ptr_tables(rsgpu_ctx* ctx, int k, int e, size_t pitch, size_t blocks, const uint8_t* d_src,
                   const uint8_t* d_par, RowPtrs& rp, size_t extra = 0);

// j: what the generated scrub, repair and locate (rs_kernels.h JitScrubArgs,
// JitRepairArgs, JitLocateArgs) launch with on the tables rp: the shared
// program of the e x k matrix `coef` (e <= 64, jit_probe(ctx) == 1; the program
// the GENERATED encode of the same matrix runs, built on first use) with the
// encode's launch settings; 16-byte aligned rows, len % 32 == 0.
int shared_epilogue_args(rsgpu_ctx* ctx, const uint8_t* coef, int k, int e, long long len, const RowPtrs& rp,
                         JitArgs& j);

// >= bytes of executable device memory at ctx->d_jit, a new generation when regrown
int jit_ensure(rsgpu_ctx* ctx, size_t bytes);

// (block, 2 KB tile) pairs below which the one-launch kernels of small batches serve
constexpr long long kTcSplitMaxWork = 2048;

// k_rs_tc over `rows` output rows in passes of <= 32, or k_rs_tc_split for a
// small batch of <= 8 rows; addr_stride elements between blocks' tables
int tc_launch(rsgpu_ctx* ctx, const char* name, const uint8_t* const* d_srcs, uint8_t* const* d_dsts,
              const unsigned long long* d_addr, long long addr_stride, int k, int rows, long long len,
              long long blocks, const int* d_status);

// v_perm table rows per source of k_dot_generic: `rows` padded to its pass
int rows_pad_for(int rows);

// the context's scratch grown to >= bytes
int ensure_scratch(rsgpu_ctx* ctx, size_t bytes);

// the fields every k_rs_tc launch fills, in TcArgs' order
inline TcArgs tc_args(const uint8_t* const* srcs, uint8_t* const* dsts, int dst_stride,
                      const unsigned long long* addr, long long addr_stride, int k, int rows, long long len,
                      const int* status)
{
    return TcArgs{srcs, dsts, dst_stride, addr, addr_stride, k, rows, len, status};
}

// the fields every generated-code launch fills (k_rs_jit, k_rs_jitw), in
// JitArgs' order: `rows` rows from dsts on, block_stride bytes between
// blocks' code (0: every block on the same code); the rest at its default
inline JitArgs jit_args(const uint8_t* const* srcs, uint8_t* const* dsts, const void* code, long long chunk_stride,
                        long long block_stride, int k, int rows, int dst_stride, long long len, const int* status)
{
    return JitArgs{srcs, dsts, (const uint8_t*)code, chunk_stride, block_stride, k, rows, dst_stride, len, status};
}

// Brackets one kernel launch with events when timing is enabled.
struct KTimer {
    rsgpu_ctx* ctx;
    hipStream_t s;
    rsgpu_ctx::Rec rec{};
    KTimer(rsgpu_ctx* c, const char* name, size_t blocks) : KTimer(c, name, blocks, c->stream) {}
    KTimer(rsgpu_ctx* c, const char* name, size_t blocks, hipStream_t st) : ctx(c), s(st)
    {
        if (!ctx->timing)
            return;
        rec.name = name;
        rec.blocks = blocks;
        rec.a = pool_event(ctx);
        rec.b = pool_event(ctx);
        (void)hipEventRecord(rec.a, s);
    }
    ~KTimer()
    {
        if (!ctx->timing)
            return;
        (void)hipEventRecord(rec.b, s);
        ctx->recs.push_back(rec);
    }
};

}  // namespace rsgpu
