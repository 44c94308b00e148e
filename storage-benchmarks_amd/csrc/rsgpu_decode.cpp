// rsgpu_decode.cpp -- the decode side of the C ABI (include/rsgpu.h):
// rsgpu_decode_blocks, rsgpu_decode_prepare / rsgpu_decode_apply,
// rsgpu_decode_general and rsgpu_verify_blocks.  Argument checks, the choice
// of a plan, the workspace layout and the launch sequences; the kernels are
// rs_kernels.hip (prepares, k_dot_generic), rs_tc.hip (threaded code),
// rs_jit.hip (generated code) and rs_bitsliced.hip (k_rs_syn_split).  Every
// entry point checks its arguments, resolves the call once (Call: geometry,
// plan, workspace view) and hands that to the functions below it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/rsgpu.h"
#include "gf256.h"
#include "jit_prog.h"
#include "rs_jit.h"
#include "rs_kernels.h"
#include "rsgpu_ctx.h"
#include "rsgpu_internal.h"

namespace {

using namespace rsgpu;

// How a decode call runs for its geometry.
enum class Plan {
    generated,   // k_decode_prepare_syn (closed form, writes code) + k_rs_jit
    one_matrix,  // k_decode_prepare_syn (closed form) + k_rs_tc
    general_tc,   // k_decode_prepare (k x k inversion) + k_rs_tc passes
    general_jit,  // k_decode_prepare + per-block generated code, passes of 32 rows
    general_dot   // k_decode_prepare + k_dot_generic (unaligned / odd lengths)
};

// column tiles (2 KB) per block from which AUTO decodes through generated
// code, every layout: the two-wave layouts (16 < e <= 32, two tiles per
// workgroup) pay from 16 tiles (C4 14.07 + 0.86 emission vs 15.44 ms
// threaded per 16384 blocks, profiles/r03_ab/c4_gen_vs_tc/), and so does the
// 8-row layout in XCD-contiguous order (per 16384 / 8192 blocks of 16 tiles,
// profiles/r03_ab/autoshort/: (64, 16) 10.69 + 0.54 vs 12.06 ms, (128, 16)
// 9.90 + 0.52 vs 11.82; round 2 measured 48 tiles, before that order); below
// kJitXcdTiles the 8-row decode runs in XCD-contiguous order
constexpr size_t kJitMinTiles = 16;
constexpr size_t kJitwMinTiles = 16;
// the general (k x k) decode through generated code in passes of 32 rows:
// no A/B below 48 tiles was made for it (round 2's threshold stays)
constexpr size_t kGeneralJitMinTiles = 48;
constexpr size_t kJitXcdTiles = 128;

size_t jit_min_tiles(int e) { return jitw_layout(e) ? kJitwMinTiles : kJitMinTiles; }

// Generated decode code of a call: two waves of 16 rows for 24 < e <= 32, of
// 12 for 20 < e <= 24, of 10 for 16 < e <= 20 (rs_jit.h Wide: the composites of a source
// built twice per tile instead of 4 or 3 times), else waves of 8 rows in
// passes of 32.  k_rs_jit16 measured on the same boxes (round 2's A/B build,
// profiles/r02_ab/jit_rows16): 10 % fewer VALU instructions, 40 % fewer
// instruction-cache misses, 3 % more cycles at 3 waves per SIMD; with the
// XCD-contiguous order 3.7 % faster than the 8-row kernel.
size_t decode_code_bytes(int k, int e, size_t blocks)
{
    return jitw_layout(e) ? jitw_code_bytes(k, e, (long long)blocks) : jit_code_bytes(k, e, (long long)blocks);
}

// generated code pays for a block of `tiles` column tiles: enough tiles to
// amortise its code (every tile's workgroup fetches all of it), or, below
// that, code small enough per tile.  (16, 8) has 10 KB per block: at 8 tiles
// (1.25 KB per tile) 3.46 + 0.15 ms emission against 3.84 threaded, at 4
// tiles (2.5 KB) 3.71 + 0.29 against 3.90, per 16 GB of sources
// (profiles/r03_ab/fewtiles/)
constexpr size_t kJitCodePerTile = 2048;
bool jit_pays(int k, int e, size_t tiles)
{
    return tiles >= jit_min_tiles(e) || decode_code_bytes(k, e, 1) <= kJitCodePerTile * tiles;
}
// (block, tile) pairs per call from which AUTO pays the emission launch
// (~10 us whatever the batch) for the ~4 ns per pair the generated code saves
// over threaded code: C2 (one block, 489 tiles) decodes 16 us threaded
// against 10 + 11 us emitted + generated (profiles/r02_ab/c2_*.json)
constexpr size_t kJitMinWork = 4096;

// the k x k general decode on aligned rows: generated code where the rows
// are long enough to amortise it (as decode_plan's AUTO), threaded code else
Plan general_plan(rsgpu_ctx* ctx, size_t len)
{
    if (tiles(len) >= kGeneralJitMinTiles && ctx->decode_kernel != RSGPU_DECODE_ONE_MATRIX && jit_probe(ctx) == 1)
        return Plan::general_jit;
    return Plan::general_tc;
}

// The plan of e rows over k sources in `blocks` blocks of `len` bytes, rows
// `aligned` (rows_aligned).  any_matrix: rsgpu_decode_general, which has no
// closed form and runs a general plan whatever the context's setting.  The
// first plan of a context probes the device (tc_handlers_ready, jit_probe).
Plan decode_plan(rsgpu_ctx* ctx, int k, int e, size_t len, size_t blocks, bool aligned, bool any_matrix)
{
    if (!aligned || !tc_handlers_ready(ctx))
        return Plan::general_dot;
    const int want = ctx->decode_kernel;
    // the closed-form rows serve every e (Lambda's e + 1 coefficients in one
    // wave up to e = 63, in LDS above); the threaded-code kernel takes e <= 32
    const bool gen_ok = !any_matrix && jit_probe(ctx) == 1 && want != RSGPU_DECODE_ONE_MATRIX &&
                        want != RSGPU_DECODE_GENERAL &&
                        (want == RSGPU_DECODE_GENERATED || jit_pays(k, e, tiles(len)));
    if (e > 32 && gen_ok)
        return Plan::generated;
    if (any_matrix || want == RSGPU_DECODE_GENERAL || e > 32)
        return general_plan(ctx, len);
    if (want == RSGPU_DECODE_ONE_MATRIX || jit_probe(ctx) != 1)
        return Plan::one_matrix;
    // AUTO: generated code only when a block has enough column tiles to
    // amortise its ~160 KB of code (every tile's workgroup fetches all of
    // it): C3 / C5 (489 tiles) 25.2 / 15.0 ms vs 27 / 17.7 threaded; L =
    // 128000 (63 tiles) 3.79 vs 3.94 ms (8-row layout, profiles/r02_ab); C4
    // (16 tiles) with two tiles per workgroup, above
    if (want == RSGPU_DECODE_AUTO && (!jit_pays(k, e, tiles(len)) || tiles(len) * blocks < kJitMinWork))
        return Plan::one_matrix;
    return Plan::generated;
}

// Workspace: [survivor ptrs B x k | output ptrs B x e | coefficient region],
// the region sized for the largest consumer: k_rs_tc handler addresses (pass
// layout), the v_perm tables, or the generated decode's e x k rows.
struct WsLayout {
    size_t surv, outp, tab, total;
};

WsLayout ws_layout(int k, int e, size_t blocks)
{
    WsLayout w{};
    size_t o = 0;
    w.surv = o;
    o = align_up(o + sizeof(void*) * (size_t)k * blocks, 256);
    w.outp = o;
    o = align_up(o + sizeof(void*) * (size_t)e * blocks, 256);
    w.tab = o;
    const size_t tc_bytes = sizeof(unsigned long long) * (size_t)tc_table_elems(k, e) * blocks;
    const size_t dot_bytes = (sizeof(uint4) + sizeof(uint32_t)) * (size_t)k * rows_pad_for(e) * blocks;
    const size_t jit_bytes = (size_t)e * k * blocks;
    w.total = align_up(o + std::max({tc_bytes, dot_bytes, jit_bytes}), 256);
    return w;
}

// A caller's workspace under that layout, typed, from block b0 on.  The
// coefficient region holds one of three things, by the call's plan.
struct Workspace {
    char* base;  // what the caller passed: the key of its generated code
    WsLayout w;
    int k, e;
    size_t blocks, b0;

    Workspace(void* d_workspace, int k_, int e_, size_t blocks_)
        : base((char*)d_workspace), w(ws_layout(k_, e_, blocks_)), k(k_), e(e_), blocks(blocks_), b0(0) {}

    Workspace from(size_t b) const
    {
        Workspace v = *this;
        v.b0 = b0 + b;
        return v;
    }
    const uint8_t** surv() const { return (const uint8_t**)(base + w.surv) + b0 * k; }  // [B][k]
    uint8_t** outp() const { return (uint8_t**)(base + w.outp) + b0 * e; }              // [B][e]
    // k_rs_tc handler addresses, tc_stride() per block (pass layout)
    unsigned long long* handlers() const { return (unsigned long long*)(base + w.tab) + b0 * tc_stride(); }
    long long tc_stride() const { return tc_table_elems(k, e); }
    // the decode rows [B][e][k] the emitters read
    uint8_t* rows() const { return (uint8_t*)(base + w.tab) + b0 * e * k; }
    // k_dot_generic's tables: tabs4 of every block, then ctab of every block,
    // dot_stride() elements per block in each
    int rows_pad() const { return rows_pad_for(e); }
    long long dot_stride() const { return (long long)k * rows_pad(); }
    uint4* tabs4() const { return (uint4*)(base + w.tab) + b0 * dot_stride(); }
    uint32_t* ctab() const
    {
        return (uint32_t*)(base + w.tab + sizeof(uint4) * (size_t)dot_stride() * blocks) + b0 * dot_stride();
    }
};

// One decode call, resolved once after its argument checks (never for e ==
// 0): m - k parity rows per block at par, e rows to rebuild into out (the
// erased originals of rsgpu_decode_blocks, where m == k + e; any nerrs rows of
// rsgpu_decode_general), the plan, and the workspace.
struct Call {
    rsgpu_ctx* ctx;
    int k, m, e;
    size_t len, pitch, blocks;
    const uint8_t *src, *par, *err;
    uint8_t* out;
    int* status;
    const uint8_t* enc;  // rsgpu_decode_general: device m x k matrix, or null for gf_gen_rs_matrix
    bool any_matrix;     // rsgpu_decode_general
    Plan plan;
    Workspace ws;
};

Call resolve(rsgpu_ctx* ctx, int k, int m, int e, size_t len, size_t pitch, size_t blocks, const uint8_t* src,
             const uint8_t* par, const uint8_t* err, uint8_t* out, void* d_workspace, int* status,
             bool any_matrix = false)
{
    const Plan plan = decode_plan(ctx, k, e, len, blocks, rows_aligned(len, pitch, src, par, out), any_matrix);
    return Call{ctx, k, m, e, len, pitch, blocks, src, par, err, out, status, nullptr, any_matrix, plan,
                Workspace(d_workspace, k, e, blocks)};
}

// The context's executable memory belongs, from now on, to the prepare of
// this (k, e, blocks, workspace): what rsgpu_decode_apply checks.
void claim_code(rsgpu_ctx* ctx, int k, int e, size_t blocks, const void* ws)
{
    ctx->jit_key.k = k;
    ctx->jit_key.e = e;
    ctx->jit_key.blocks = blocks;
    ctx->jit_key.ws = ws;
    ctx->jit_key.gen = ++ctx->jit_gen;
}

const char* emit_name(int e)
{
    if (!jitw_layout(e))
        return "k_jit_emit";
    const int r = jitw_rows(jit::wide_pass_rows(e, 0));
    return r == 16 ? "k_jit16_emit" : r == 12 ? "k_jit12_emit" : "k_jit10_emit";
}

// k_jit_emit / k_jitw_emit on stream st: the code of blocks [b0, b0 + nb)
// from their decode rows in the workspace, each block's at its place in the
// call's code
int launch_emit(const Call& c, size_t b0, size_t nb, hipStream_t st)
{
    const uint8_t* rows = c.ws.from(b0).rows();
    uint8_t* code = (uint8_t*)c.ctx->d_jit + b0 * decode_code_bytes(c.k, c.e, 1);
    KTimer ke(c.ctx, emit_name(c.e), nb, st);
    if (jitw_layout(c.e))
        RS_HIP(c.ctx, launch_jitw_emit(c.k, c.e, (long long)nb, rows, c.status + b0, code, st));
    else
        RS_HIP(c.ctx, launch_jit_emit(c.k, c.e, (long long)nb, rows, c.status + b0, code, st));
    return RSGPU_OK;
}

// k_decode_prepare_syn on stream st for blocks [b0, b0 + nb): row pointers,
// and the closed-form rows as handler addresses (one_matrix) or as they are
// (generated: the emitters read them from the coefficient region)
int launch_prepare_syn(const Call& c, size_t b0, size_t nb, hipStream_t st)
{
    const bool gen = c.plan == Plan::generated;
    const Workspace w = c.ws.from(b0);
    KTimer kt(c.ctx, "k_decode_prepare_syn", nb, st);
    RS_HIP(c.ctx, launch_decode_prepare_syn(c.k, c.e, (long long)nb, c.err + b0 * c.e, c.out + b0 * c.e * c.pitch,
                                            (long long)c.pitch, w.surv(), w.outp(), c.ctx->d_tc_table, c.status + b0,
                                            c.src + b0 * c.k * c.pitch, c.par + b0 * c.e * c.pitch,
                                            gen ? nullptr : w.handlers(), gen ? w.rows() : nullptr, st));
    return RSGPU_OK;
}

// k_rs_jitw on stream st over blocks [b0, b0 + nb) of the call's code, one
// launch per pass of <= 64 rows (one pass for e <= 64)
int jitw_launch(const Call& c, size_t b0, size_t nb, hipStream_t st)
{
    rsgpu_ctx* ctx = c.ctx;
    const int k = c.k, e = c.e;
    const Workspace w = c.ws.from(b0);
    const size_t bs = jitw_code_bytes(k, e, 1);
    const uint8_t* code = (const uint8_t*)ctx->d_jit + b0 * bs;
    for (int p = 0; p < jit::wide_passes(e); ++p) {
        const int rows = jit::wide_pass_rows(e, p);
        JitArgs j = jit_args(w.surv(), w.outp() + jit::wide_pass_row0(e, p), code + jitw_pass_offset(k, e, p),
                             (long long)jitw_chunk_stride(rows), (long long)bs, k, rows, e, (long long)c.len,
                             c.status + b0);
        // each XCD a contiguous range of (block, tile): a block's code is
        // fetched into one L2, not eight -- 3.7 % faster at C3 for the
        // 16-row kernel (23.3 vs 24.2 ms, profiles/r02_ab/jit_rows16/xcd_*.log),
        // where the 8-row kernel measured 1 % slower
        j.xcd_order = 1;
        // two column tiles per workgroup: the waves with the same rows share
        // their code's instruction-cache lines (C4 13.7 vs 14.2 ms per 16384
        // blocks, C3 23.2-23.3 vs 23.4-23.5, C5 12.7-12.8 vs 12.8-12.9;
        // three tiles: 20-30 % slower; profiles/r03_ab/tpw/)
        j.tiles_per_wg = jit::wide_waves(rows) == 4 ? 1 : ctx->jitw_tpw ? ctx->jitw_tpw : 2;
        // short rows: the block's few workgroups pull its code into L2 before
        // the instruction fetch misses on it line by line (C4: 12.8 vs 13.7
        // ms per 16384 blocks; C3, 245 workgroups per block, unchanged:
        // profiles/r03_ab/prefetch/)
        {
            const long long wgs = ((long long)tiles(c.len) + j.tiles_per_wg - 1) / j.tiles_per_wg;
            const long long lines = (long long)jitw_pass_bytes(k, rows) / 128;
            j.code_prefetch = ctx->jitw_prefetch >= 0 ? ctx->jitw_prefetch : lines >= 32 * wgs;
        }
        // chunk order rotated by each workgroup's start time, so the
        // workgroups sharing a CU pair's instruction cache walk their block's
        // code in step (k_rs_jitw).  Not for short rows: a block's few
        // workgroups run its code once each, and the rotation measured +0.5 %
        // on the C4 step (same-process ABBA x6, profiles/r05_rot/shared/)
        j.chunk_rot_ticks = ctx->jitw_rot >= 0 ? ctx->jitw_rot : j.code_prefetch ? 0 : jitw_rot_ticks(rows);
        j.prio = ctx->jitw_prio;
        const int r = jitw_rows(rows);
        KTimer kt(ctx,
                  e > 64  ? "k_rs_jitw_passes(decode)"
                  : e > 32 ? (r == 16 ? "k_rs_jit16x4(decode)" : r == 12 ? "k_rs_jit12x4(decode)" : "k_rs_jit10x4(decode)")
                  : r == 16 ? "k_rs_jit16(decode)"
                  : r == 12 ? "k_rs_jit12(decode)"
                            : "k_rs_jit10(decode)",
                  nb, st);
        RS_HIP(ctx, launch_rs_jitw(j, (long long)nb, st));
    }
    return RSGPU_OK;
}

// The per-block generated decode (rs_jit.hip) over rows e of every block:
// k_rs_jitw in one launch (decode_code_bytes), or k_rs_jit in passes of
// <= 32 rows: block b, pass p, wave w, chunk ch at d_jit + b block_stride +
// ((4 p + w) nch + ch) chunk_stride (k_jit_emit's layout).
int jit_decode_launch(const Call& c)
{
    rsgpu_ctx* ctx = c.ctx;
    const int k = c.k, e = c.e;
    if (!ctx->d_jit || ctx->jit_bytes < decode_code_bytes(k, e, c.blocks))
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_decode_apply: no prepared decode code");
    // the code must be the one this workspace's prepare emitted, untouched
    // since: another prepare, a decode_general or a regrow rewrites it
    if (ctx->jit_key.gen != ctx->jit_gen || ctx->jit_key.k != k || ctx->jit_key.e != e ||
        ctx->jit_key.blocks != c.blocks || ctx->jit_key.ws != c.ws.base)
        return fail(ctx, RSGPU_ERR_ARG,
                    "rsgpu_decode_apply: the generated code belongs to another prepare "
                    "(re-run rsgpu_decode_prepare for this workspace)");
    if (jitw_layout(e))
        return jitw_launch(c, 0, c.blocks, ctx->stream);
    const int nch = (k + 7) / 8, nwt = (e + 7) / 8;
    for (int p = 0; p * 32 < e; ++p) {
        JitArgs j = jit_args(c.ws.surv(), c.ws.outp() + 32 * p,
                             (const uint8_t*)ctx->d_jit + (size_t)4 * p * nch * jit::chunk_stride(8),
                             jit::chunk_stride(8), (long long)nwt * nch * jit::chunk_stride(8), k,
                             std::min(32, e - 32 * p), e, (long long)c.len, c.status);
        // few tiles per block: keep each block's code in one XCD's L2
        j.xcd_order = tiles(c.len) < kJitXcdTiles;
        j.prio = ctx->jitw_prio;
        KTimer kt(ctx, "k_rs_jit(decode)", c.blocks);
        RS_HIP(ctx, launch_rs_jit(j, (long long)c.blocks, ctx->stream));
    }
    return RSGPU_OK;
}

// k_decode_prepare launch for the general plans
int general_prepare(const Call& c)
{
    rsgpu_ctx* ctx = c.ctx;
    PrepArgs p{};
    p.k = c.k;
    p.m = c.m;
    p.nerrs = c.e;
    p.rows_pad = c.ws.rows_pad();
    p.blocks = (long long)c.blocks;
    p.err = c.err;
    p.enc = c.enc;
    p.originals_only = c.any_matrix ? 0 : 1;
    p.src = c.src;
    p.src_pitch = (long long)c.pitch;
    p.par = c.par;
    p.par_pitch = (long long)c.pitch;
    p.out = c.out;
    p.out_pitch = (long long)c.pitch;
    p.surv_ptrs = c.ws.surv();
    p.out_ptrs = c.ws.outp();
    p.status = c.status;
    if (c.plan == Plan::general_jit) {
        p.coef_out = c.ws.rows();
        const int rc = jit_ensure(ctx, decode_code_bytes(c.k, c.e, c.blocks));
        if (rc)
            return rc;
    } else if (c.plan == Plan::general_tc) {
        p.tc_table = ctx->d_tc_table;
        p.tc_addr = c.ws.handlers();
        p.tc_block_stride = c.ws.tc_stride();
    } else {
        p.tabs4 = c.ws.tabs4();
        p.ctab = c.ws.ctab();
        p.tab_block_stride = c.ws.dot_stride();
    }
    {
        KTimer kt(ctx, "k_decode_prepare", c.blocks);
        RS_HIP(ctx, launch_decode_prepare(p, ctx->stream));
    }
    if (c.plan == Plan::general_jit) {
        claim_code(ctx, c.k, c.e, c.blocks, c.ws.base);
        return launch_emit(c, 0, c.blocks, ctx->stream);
    }
    return RSGPU_OK;
}

// What rsgpu_decode_prepare enqueues: the row pointers and the decode rows of
// every block, in the form the call's plan applies.
int prepare(const Call& c)
{
    rsgpu_ctx* ctx = c.ctx;
    if (c.plan != Plan::one_matrix && c.plan != Plan::generated)
        return general_prepare(c);
    const bool gen = c.plan == Plan::generated;
    if (gen) {
        const int rc = jit_ensure(ctx, decode_code_bytes(c.k, c.e, c.blocks));
        if (rc)
            return rc;
    }
    const int rc = launch_prepare_syn(c, 0, c.blocks, ctx->stream);
    if (rc || !gen)
        return rc;
    claim_code(ctx, c.k, c.e, c.blocks, c.ws.base);
    return launch_emit(c, 0, c.blocks, ctx->stream);
}

// What rsgpu_decode_apply enqueues (len > 0): the rows of every block with
// status 0, from what prepare(c) left in the workspace.
int apply(const Call& c)
{
    if (c.plan == Plan::generated || c.plan == Plan::general_jit)
        // the block's generated code (rs_jit.hip)
        return jit_decode_launch(c);
    if (c.plan == Plan::one_matrix || c.plan == Plan::general_tc)
        // one matrix over the survivors: one pass up to 32 rows
        return tc_launch(c.ctx, "k_rs_tc(decode)", c.ws.surv(), c.ws.outp(), c.ws.handlers(), c.ws.tc_stride(), c.k,
                         c.e, (long long)c.len, (long long)c.blocks, c.status);
    DotArgs a{};
    a.srcs = c.ws.surv();
    a.dsts = c.ws.outp();
    a.tabs4 = c.ws.tabs4();
    a.ctab = c.ws.ctab();
    a.tab_block_stride = c.ws.dot_stride();
    a.k = c.k;
    a.rows = c.e;
    a.rows_pad = c.ws.rows_pad();
    a.len = (long long)c.len;
    a.blocks = (long long)c.blocks;
    a.status = c.status;
    a.bytewise = !ptrs_aligned(c.pitch, c.src, c.par, c.out);
    KTimer kt(c.ctx, "k_dot_generic(decode)", c.blocks);
    RS_HIP(c.ctx, launch_dot_generic(a, c.ctx->stream));
    return RSGPU_OK;
}

// A small batch of the one-matrix decode with few rows (C2: one block of
// (16, 4, 1e6)): the decode rows are built inside the decode kernel, one
// launch instead of prepare + apply, and no workspace
bool small_shape(int k, int e, size_t len, size_t blocks)
{
    return e <= 8 && k <= 64 && len > 0 && (long long)(tiles(len) * blocks) < kTcSplitMaxWork;
}

int decode_small(const Call& c)
{
    rsgpu_ctx* ctx = c.ctx;
    // AUTO, and a code with a compiled single-chunk program (C2's (16, 4)):
    // syndromes through the compiled programs, the e x e solve in the same
    // launch (k_rs_syn_split); otherwise the threaded-code one-launch decode
    if (ctx->decode_kernel == RSGPU_DECODE_AUTO && rs_bitsliced_split_available(c.k, c.e)) {
        SynArgs y{};
        y.src = c.src;
        y.par = c.par;
        y.out = c.out;
        y.err = c.err;
        y.status = c.status;
        y.pitch = (long long)c.pitch;
        y.len = (long long)c.len;
        KTimer kt(ctx, "k_rs_syn_split(decode)", c.blocks);
        RS_HIP(ctx, launch_rs_syn_split(c.k, c.e, y, (long long)c.blocks, ctx->stream));
        return RSGPU_OK;
    }
    TcFusedArgs f{};
    f.k = c.k;
    f.e = c.e;
    f.len = (long long)c.len;
    f.pitch = (long long)c.pitch;
    f.blocks = (long long)c.blocks;
    f.err = c.err;
    f.src = c.src;
    f.par = c.par;
    f.out = c.out;
    f.status = c.status;
    f.map_base = ctx->tc_base;
    f.map_stride = tc_handler_stride();
    for (int sl = 0; sl < 8; ++sl)
        f.map_copy[sl] = tc_slot_copy(sl);
    KTimer kt(ctx, "k_rs_tc_fused(decode)", c.blocks);
    RS_HIP(ctx, launch_rs_tc_fused(f, ctx->stream));
    return RSGPU_OK;
}

// Short-row batches of the generated decode (C4: 16 column tiles per block,
// 16384 blocks per call): run first on the context's stream, the prepare and
// the code emission of the whole batch (0.26 + 0.63 ms per C4 batch) hide
// behind no kernel.  Here the batch goes in `parts` slices of whole blocks:
// every slice's prepare and emission run on a second stream, and the context's
// stream waits for a slice's code just before that slice's decode launch, so
// the later slices' emission runs beside the earlier slices' decode.  Each
// slice's code has its place in the batch's code (block b at b x the block
// stride) and the workspace's key is the batch's: the result and the state
// left behind are those of prepare + apply.
constexpr size_t kPipeMinBlocks = 2048;
constexpr size_t kPipeMaxTiles = 64;
constexpr int kPipeParts = 4;

int decode_parts(const Call& c)
{
    if (c.plan != Plan::generated || !jitw_layout(c.e) || c.blocks < 4 || c.len == 0)
        return 1;
    if (c.ctx->decode_pipe >= 0)
        return std::max(1, std::min(c.ctx->decode_pipe, (int)(c.blocks / 2)));
    return tiles(c.len) <= kPipeMaxTiles && c.blocks >= kPipeMinBlocks ? kPipeParts : 1;
}

int decode_slices(const Call& c, int parts)
{
    rsgpu_ctx* ctx = c.ctx;
    claim_code(ctx, c.k, c.e, c.blocks, c.ws.base);
    // the second stream starts behind everything enqueued on the context's
    // stream so far (the erasure lists, the code memory's fill, the kernels
    // of the last call that read this workspace and code)
    hipEvent_t start = sync_event(ctx);
    RS_HIP(ctx, hipEventRecord(start, ctx->stream));
    RS_HIP(ctx, hipStreamWaitEvent(ctx->aux, start, 0));
    // slices of an even number of blocks: a slice's code starts on a 128-byte line
    const size_t per = ((c.blocks + parts - 1) / parts + 1) / 2 * 2;
    for (size_t b0 = 0; b0 < c.blocks; b0 += per) {
        const size_t nb = std::min(per, c.blocks - b0);
        int rc = launch_prepare_syn(c, b0, nb, ctx->aux);
        if (!rc)
            rc = launch_emit(c, b0, nb, ctx->aux);
        if (rc)
            return rc;
        hipEvent_t ready = sync_event(ctx);
        RS_HIP(ctx, hipEventRecord(ready, ctx->aux));
        RS_HIP(ctx, hipStreamWaitEvent(ctx->stream, ready, 0));
        rc = jitw_launch(c, b0, nb, ctx->stream);
        if (rc)
            return rc;
    }
    return RSGPU_OK;
}

int decode_pipelined(const Call& c, int parts)
{
    rsgpu_ctx* ctx = c.ctx;
    const int rc = jit_ensure(ctx, decode_code_bytes(c.k, c.e, c.blocks));
    if (rc)
        return rc;
    if (!ctx->aux)
        RS_HIP(ctx, rsgpu_ctx_stream_create(ctx, &ctx->aux));
    const int rs = decode_slices(c, parts);
    if (rs)
        ctx->jit_key.gen = 0;  // a failed call leaves no prepare behind for an apply to trust
    // whatever the outcome, nothing enqueued on the second stream outlives
    // the context's stream order (a failed launch leaves no emission behind
    // that later work on the same code or workspace could race)
    hipEvent_t done = sync_event(ctx);
    if (hipEventRecord(done, ctx->aux) != hipSuccess || hipStreamWaitEvent(ctx->stream, done, 0) != hipSuccess) {
        (void)hipStreamSynchronize(ctx->aux);
        return rs ? rs : fail(ctx, RSGPU_ERR_HIP, "rsgpu_decode_blocks: joining the emission stream");
    }
    return rs;
}

// rsgpu_decode_blocks on at most kMaxGridBlocks blocks, e > 0: the
// single-launch small decode, the pipelined slices, or prepare + apply
int decode_slice(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks, const uint8_t* d_src,
                 const uint8_t* d_parity, const uint8_t* d_err, uint8_t* d_out, void* d_workspace, int* d_status)
{
    const bool small = small_shape(k, e, len, blocks);
    if (!d_workspace && !small)  // what prepare + apply would answer, before any plan is made
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_decode_prepare: bad arguments");
    const Call c = resolve(ctx, k, k + e, e, len, pitch, blocks, d_src, d_parity, d_err, d_out, d_workspace, d_status);
    if (small && c.plan == Plan::one_matrix)
        return decode_small(c);
    if (!d_workspace)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_decode_prepare: bad arguments");
    // short rows, many blocks: prepare and emission beside the decode
    if (const int parts = decode_parts(c); parts > 1)
        return decode_pipelined(c, parts);
    const int rc = prepare(c);
    return rc || len == 0 ? rc : apply(c);
}

// rsgpu_decode_general on at most kMaxGridBlocks blocks, nerrs > 0
int decode_general_slice(rsgpu_ctx* ctx, int k, int m, size_t len, size_t pitch, size_t blocks,
                         const unsigned char* encode_matrix, const uint8_t* d_src, const uint8_t* d_parity,
                         const uint8_t* d_err, int nerrs, uint8_t* d_out, void* d_workspace, int* d_status)
{
    Call c = resolve(ctx, k, m, nerrs, len, pitch, blocks, d_src, d_parity, d_err, d_out, d_workspace, d_status, true);
    if (encode_matrix) {
        const size_t bytes = (size_t)m * k;
        int rc = ensure_scratch(ctx, bytes);
        if (rc)
            return rc;
        void* stage;
        rc = get_stage(ctx, bytes, &stage);
        if (rc)
            return rc;
        std::memcpy(stage, encode_matrix, bytes);
        rc = upload(ctx, ctx->scratch.p, bytes);
        if (rc)
            return rc;
        c.enc = (const uint8_t*)ctx->scratch.p;
    }
    const int rc = prepare(c);
    return rc || len == 0 ? rc : apply(c);
}

}  // namespace

extern "C" {

int rsgpu_set_decode_kernel(rsgpu_ctx* ctx, int kernel)
{
    if (!ctx || kernel < RSGPU_DECODE_AUTO || kernel > RSGPU_DECODE_GENERATED)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_set_decode_kernel: unknown kernel");
    // the retired FUSED choice runs ONE_MATRIX (the same bytes; rsgpu.h)
    ctx->decode_kernel = kernel == RSGPU_DECODE_FUSED ? RSGPU_DECODE_ONE_MATRIX : kernel;
    return RSGPU_OK;
}

size_t rsgpu_decode_workspace_bytes(int k, int e, size_t blocks)
{
    if (k <= 0 || e <= 0)
        return 256;
    return ws_layout(k, e, blocks).total;
}

int rsgpu_decode_prepare(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                         const unsigned char* d_src, const unsigned char* d_parity,
                         const unsigned char* d_err, unsigned char* d_out, void* d_workspace,
                         int* d_status)
{
    int rc = check_geom(ctx, k, e, len, pitch, blocks);
    if (rc)
        return rc;
    if (e == 0)
        return RSGPU_OK;
    if (e > k || !d_err || !d_workspace || !d_status)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_decode_prepare: bad arguments");
    if (blocks > kMaxGridBlocks)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_decode_prepare: at most 65535 blocks per call "
                                        "(rsgpu_decode_blocks slices larger batches)");
    return prepare(resolve(ctx, k, k + e, e, len, pitch, blocks, d_src, d_parity, d_err, d_out, d_workspace, d_status));
}

int rsgpu_decode_apply(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                       const unsigned char* d_src, const unsigned char* d_parity,
                       unsigned char* d_out, void* d_workspace, const int* d_status)
{
    int rc = check_geom(ctx, k, e, len, pitch, blocks);
    if (rc)
        return rc;
    if (e == 0 || len == 0)
        return RSGPU_OK;
    if (e > k || !d_workspace || !d_status)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_decode_apply: bad arguments");
    if (blocks > kMaxGridBlocks)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_decode_apply: at most 65535 blocks per call "
                                        "(rsgpu_decode_blocks slices larger batches)");
    // apply only reads the statuses
    return apply(resolve(ctx, k, k + e, e, len, pitch, blocks, d_src, d_parity, nullptr, d_out, d_workspace,
                         const_cast<int*>(d_status)));
}

int rsgpu_decode_blocks(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                        const unsigned char* d_src, const unsigned char* d_parity,
                        const unsigned char* d_err, unsigned char* d_out, void* d_workspace,
                        int* d_status)
{
    int rc = check_geom(ctx, k, e, len, pitch, blocks);
    if (rc)
        return rc;
    if (e == 0)
        return RSGPU_OK;
    if (e > k || !d_err || !d_status)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_decode_blocks: bad arguments");
    // slices in stream order, each planned on its own and through the start
    // of the workspace (a slice's layout is no larger than the whole batch's)
    return for_grid_slices(blocks, [&](size_t b0, size_t nb) {
        return decode_slice(ctx, k, e, len, pitch, nb, d_src + b0 * k * pitch, d_parity + b0 * e * pitch,
                            d_err + b0 * e, d_out + b0 * e * pitch, d_workspace, d_status + b0);
    });
}

size_t rsgpu_decode_general_workspace_bytes(int k, int m, int nerrs, size_t blocks)
{
    if (k <= 0 || m < k || nerrs <= 0)
        return 256;
    return ws_layout(k, nerrs, blocks).total;
}

int rsgpu_decode_general(rsgpu_ctx* ctx, int k, int m, size_t len, size_t pitch, size_t blocks,
                         const unsigned char* encode_matrix, const unsigned char* d_src,
                         const unsigned char* d_parity, const unsigned char* d_err, int nerrs,
                         unsigned char* d_out, void* d_workspace, int* d_status)
{
    int rc = check_geom(ctx, k, m - k, len, pitch, blocks);
    if (rc)
        return rc;
    if (nerrs < 0 || nerrs > m - k)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_decode_general: nerrs must be in [0, m - k]");
    if (nerrs == 0)
        return RSGPU_OK;
    if (!d_err || !d_workspace || !d_status || !d_out)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_decode_general: bad arguments");
    return for_grid_slices(blocks, [&](size_t b0, size_t nb) {
        return decode_general_slice(ctx, k, m, len, pitch, nb, encode_matrix, d_src + b0 * k * pitch,
                                    d_parity + b0 * (m - k) * pitch, d_err + b0 * nerrs, nerrs,
                                    d_out + b0 * nerrs * pitch, d_workspace, d_status + b0);
    });
}

int rsgpu_verify_blocks(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                        const unsigned char* d_src, const unsigned char* d_out,
                        const unsigned char* d_err, unsigned long long* d_mismatch)
{
    int rc = check_geom(ctx, k, e, len, pitch, blocks);
    if (rc)
        return rc;
    if (e == 0 || len == 0)
        return RSGPU_OK;
    return for_grid_slices(blocks, [&](size_t b0, size_t nb) {
        RS_HIP(ctx, launch_compare_rows(d_src + b0 * k * pitch, (long long)pitch, k, d_out + b0 * e * pitch,
                                        (long long)pitch, e, d_err + b0 * e, (long long)len, (long long)nb,
                                        d_mismatch + b0, ctx->stream));
        return (int)RSGPU_OK;
    });
}

}  // extern "C"
