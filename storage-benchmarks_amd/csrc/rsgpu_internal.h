// rsgpu_internal.h -- host helpers that rsgpu_capi.cpp defines and the other
// host files of librsgpu share (rsgpu_scrub.cpp).  Internal: rsgpu.map keeps
// all of it out of the library's exports.
#pragma once
#include "gf256.h"
#include "rsgpu_ctx.h"

namespace rsgpu {

const GfTables& host_gf();
uint8_t hmul(uint8_t a, uint8_t b);

// the argument check every block-batched entry point starts with
int check_geom(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks);

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

// the handler table of k_rs_tc (rs_tc.hip) is located and ctx->d_tc_table holds
// its addresses; probed once per context
bool tc_handlers_ready(rsgpu_ctx* ctx);

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
