// rsgpu_capi.cpp -- C ABI of librsgpu (include/rsgpu.h): host GF helpers with
// ISA-L semantics, context/stream management, the ISA-L-shaped device calls,
// the launch sequence of the batched encode, and the infrastructure the encode
// and the decode share (handler table, executable memory, shared programs,
// k_rs_tc launches).  The decode is rsgpu_decode.cpp; scrub, repair, update,
// degraded scrub and rebuild are rsgpu_scrub.cpp; what the three files share
// is declared in rsgpu_internal.h.
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rsgpu.h"
#include "gf256.h"
#include "rsgpu_ctx.h"
#include "rsgpu_internal.h"
#include "jit_prog.h"
#include "rs_jit.h"
#include "rs_kernels.h"
#include "rs_synth.h"

namespace {

using namespace rsgpu;

// Locate the handler table of k_rs_tc once per context: the query kernel
// reports the table's first and end addresses; the layout must be exactly
// tc_handler_count() handlers of tc_handler_stride() bytes, otherwise the
// threaded-code path stays off (and k_dot_generic serves).  The address
// table has 2048 entries: [slot][coefficient], each the handler copy that
// serves the slot (tc_slot_copy).
int tc_init(rsgpu_ctx* ctx)
{
    if (ctx->tc_state != 0)
        return ctx->tc_state;
    ctx->tc_state = -1;
    unsigned long long* d = nullptr;
    if (hipMalloc((void**)&d, 2050 * sizeof(unsigned long long)) != hipSuccess)
        return -1;
    unsigned long long se[2] = {0, 0};
    if (tc_query_handlers(d + 2048, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(se, d + 2048, sizeof se, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {
        (void)hipFree(d);
        return -1;
    }
    const unsigned long long stride = (unsigned long long)tc_handler_stride();
    const unsigned long long count = (unsigned long long)tc_handler_count();
    if (se[0] == 0 || se[1] - se[0] != count * stride || count % 256 != 0 || count > 2048) {
        std::fprintf(stderr, "rsgpu: threaded-code handler table has an unexpected layout "
                             "(%#llx..%#llx); using k_dot_generic\n", se[0], se[1]);
        (void)hipFree(d);
        return -1;
    }
    unsigned long long h[2048];
    for (int s = 0; s < 8; ++s)
        for (int c = 0; c < 256; ++c)
            h[s * 256 + c] = se[0] + (unsigned long long)(tc_slot_copy(s) * 256 + c) * stride;
    if (hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return -1;
    }
    std::memcpy(ctx->h_tc_table, h, sizeof h);
    ctx->tc_base = se[0];
    ctx->d_tc_table = d;
    ctx->tc_state = 1;
    return 1;
}

hsa_status_t pick_coarse_pool(hsa_amd_memory_pool_t p, void* out)
{
    hsa_amd_segment_t seg;
    if (hsa_amd_memory_pool_get_info(p, HSA_AMD_MEMORY_POOL_INFO_SEGMENT, &seg) != HSA_STATUS_SUCCESS ||
        seg != HSA_AMD_SEGMENT_GLOBAL)
        return HSA_STATUS_SUCCESS;
    uint32_t flags = 0;
    bool alloc = false;
    hsa_amd_memory_pool_get_info(p, HSA_AMD_MEMORY_POOL_INFO_GLOBAL_FLAGS, &flags);
    hsa_amd_memory_pool_get_info(p, HSA_AMD_MEMORY_POOL_INFO_RUNTIME_ALLOC_ALLOWED, &alloc);
    if ((flags & HSA_AMD_MEMORY_POOL_GLOBAL_FLAG_COARSE_GRAINED) && alloc) {
        *(hsa_amd_memory_pool_t*)out = p;
        return HSA_STATUS_INFO_BREAK;
    }
    return HSA_STATUS_SUCCESS;
}

// The shared program of a matrix (jit_prog.h, composites by greedy cover):
// for 16 < rows <= 64 in the two- / four-wave layout of the decode (k_rs_jitw: a
// source's composites built twice or four times per tile), above 64 rows in
// passes of <= 64 in that layout (one program per pass, concatenated), else
// the 8-row layout (k_rs_jit).  Built on the host (~50 us for one row of 32
// sources, ~0.3 ms for 32 x 32) and kept in a per-context LRU cache of up to
// kProgCacheEntries programs / kProgCacheBytes, so a caller cycling through a
// few matrices (isa_arithmetic's one-output-per-call loop: 32 rows) builds
// each once.  Each program has its own executable buffer; an eviction waits
// for the context's stream first (a kernel in flight may run that code).
constexpr size_t kProgCacheEntries = 64;
constexpr size_t kProgCacheBytes = 256u << 20;

// kara: the Karatsuba-split program of the (64, 32) gf_gen_rs_matrix code
// (jit_prog.h build_karatsuba_code; k_rs_kara) instead, cached the same way.
const rsgpu_ctx::SharedProg* shared_program(rsgpu_ctx* ctx, const uint8_t* coef, int k, int rows, int* rc_out,
                                            bool kara = false)
{
    *rc_out = RSGPU_OK;
    const bool wide = jitw_layout(rows);
    std::vector<uint8_t> key(9 + (size_t)k * rows);
    std::memcpy(key.data(), &k, 4);
    std::memcpy(key.data() + 4, &rows, 4);
    key[8] = kara ? 2 : wide ? 1 : 0;
    std::memcpy(key.data() + 9, coef, (size_t)k * rows);
    for (auto& pr : ctx->progs)
        if (pr.key == key) {
            pr.last = ++ctx->prog_tick;
            return &pr;
        }
    auto err = [&](int code, const char* msg) -> const rsgpu_ctx::SharedProg* {
        *rc_out = fail(ctx, code, msg);
        return nullptr;
    };
    if (jit_probe(ctx) != 1)
        return err(RSGPU_ERR_UNSUPPORTED, "no executable device memory pool");
    int stride = 0;
    std::vector<uint8_t> code;
    std::vector<std::pair<size_t, int>> passes;
    if (kara) {
        jit::KaraProgram kp;
        if (k != 64 || rows != 32 || !jit::build_karatsuba_code(coef, &kp))
            return err(RSGPU_ERR_UNSUPPORTED, "Karatsuba program: not the (64, 32) gf_gen_rs_matrix code");
        code = std::move(kp.code);
        stride = kp.chunk_stride;
    } else if (wide) {
        code = jit::build_matrix_code_wide_passes(coef, k, rows, &passes);
        if (code.empty())
            return err(RSGPU_ERR_UNSUPPORTED, "shared program: rows exceed the layout");
    } else {
        code = jit::build_matrix_code(coef, k, rows, &stride);
    }
    // room: least recently used programs out, after the stream has drained
    size_t used = 0;
    for (const auto& pr : ctx->progs)
        used += pr.bytes;
    if (!ctx->progs.empty() &&
        (ctx->progs.size() >= kProgCacheEntries || used + code.size() > kProgCacheBytes)) {
        if (hipStreamSynchronize(ctx->stream) != hipSuccess)
            return err(RSGPU_ERR_HIP, "shared program: draining the stream before an eviction");
        while (!ctx->progs.empty() &&
               (ctx->progs.size() >= kProgCacheEntries || used + code.size() > kProgCacheBytes)) {
            auto lru = std::min_element(ctx->progs.begin(), ctx->progs.end(),
                                        [](const auto& a, const auto& b) { return a.last < b.last; });
            used -= lru->bytes;
            hsa_amd_memory_pool_free(lru->code);
            ctx->progs.erase(lru);
        }
    }
    if (ctx->code_stage_bytes < code.size()) {
        if (hipStreamSynchronize(ctx->stream) != hipSuccess)
            return err(RSGPU_ERR_HIP, "shared program: draining the stream before regrowing the stage");
        if (ctx->d_code_stage)
            (void)hipFree(ctx->d_code_stage);
        ctx->d_code_stage = nullptr;
        ctx->code_stage_bytes = 0;
        if (hipMalloc(&ctx->d_code_stage, code.size()) != hipSuccess)
            return err(RSGPU_ERR_NOMEM, "shared program: code stage allocation failed");
        ctx->code_stage_bytes = code.size();
    }
    rsgpu_ctx::SharedProg pr;
    if (hsa_amd_memory_pool_allocate(ctx->jit_pool, code.size(), HSA_AMD_MEMORY_POOL_EXECUTABLE_FLAG,
                                     &pr.code) != HSA_STATUS_SUCCESS || !pr.code)
        return err(RSGPU_ERR_NOMEM, "executable device allocation failed");
    pr.bytes = code.size();
    void* stage;
    int rc = get_stage(ctx, code.size(), &stage);
    if (!rc) {
        std::memcpy(stage, code.data(), code.size());
        rc = upload(ctx, ctx->d_code_stage, code.size());
    }
    if (!rc && launch_jit_copy(pr.code, ctx->d_code_stage, code.size(), ctx->stream) != hipSuccess)
        rc = fail(ctx, RSGPU_ERR_HIP, "shared program: copy into executable memory");
    if (rc) {
        hsa_amd_memory_pool_free(pr.code);
        *rc_out = rc;
        return nullptr;
    }
    pr.key = std::move(key);
    pr.chunk_stride = stride;
    pr.passes = std::move(passes);
    pr.last = ++ctx->prog_tick;
    ctx->progs.push_back(std::move(pr));
    return &ctx->progs.back();
}

// The launch arguments of pass p of the shared program pg of `rows` rows, on
// the row pointers d_srcs [B][k] and d_dsts [B][rows]: a pass of <= 64 rows of
// the two- / four-wave kernel (jitw_layout(rows)), else of <= 32 rows of the
// 8-row kernel; every block on the same code.  The encode and the generated
// scrub launch with these settings.
JitArgs shared_pass_args(const rsgpu_ctx* ctx, const rsgpu_ctx::SharedProg* pg, int k, int rows, int p,
                         long long len, const uint8_t* const* d_srcs, uint8_t* const* d_dsts)
{
    if (jitw_layout(rows)) {
        JitArgs j = jit_args(d_srcs, d_dsts + jit::wide_pass_row0(rows, p),
                             (const uint8_t*)pg->code + pg->passes[p].first, pg->passes[p].second, 0, k,
                             jit::wide_pass_rows(rows, p), rows, len, nullptr);
        j.tiles_per_wg = ctx->jitw_tpw ? ctx->jitw_tpw : 2;
        // every block on the same code: the start-time chunk rotation
        // (k_rs_jitw) lines up the workgroups of a CU pair on one chunk
        // (same-process ABBA x6, profiles/r05_rot/shared/: C5 encode 12.96
        // -> 12.37 ms, step -2.7 %; (48, 24) step -0.7 %; C3's generated
        // encode 22.65 -> 21.73 ms, still 1.7 % behind k_rs_bs)
        j.chunk_rot_ticks = ctx->jitw_rot >= 0 ? ctx->jitw_rot : jitw_rot_ticks(j.rows);
        j.prio = ctx->jitw_prio;
        return j;
    }
    const int nch = (k + 7) / 8;
    JitArgs j = jit_args(d_srcs, d_dsts + 32 * p, (const uint8_t*)pg->code + (size_t)p * 4 * nch * pg->chunk_stride,
                         pg->chunk_stride, 0, k, std::min(32, rows - 32 * p), rows, len, nullptr);
    // no wave priority for the shared 8-row program: (32, 8)'s encode
    // measured 15.25 -> 17.06 ms with it, (8, 2)'s +1 % (same process
    // ABBA x6, profiles/r06_prio/r06_prio_small_e/); the per-block 8-row
    // decode keeps it (16, 4) -1.4 %, (64, 16) -3.2 %
    j.prio = 0;
    return j;
}

// dsts[b][i] = sum_j coef[i][j] srcs[b][j] through the shared generated code,
// in passes of <= 32 rows (aligned rows, len % 32 == 0)
int shared_program_launch(rsgpu_ctx* ctx, const uint8_t* coef, int k, int rows, long long len,
                          long long blocks, const uint8_t* const* d_srcs, uint8_t* const* d_dsts,
                          const char* name)
{
    int rc = RSGPU_OK;
    const rsgpu_ctx::SharedProg* pg = shared_program(ctx, coef, k, rows, &rc);
    if (!pg)
        return rc;
    const bool wide = jitw_layout(rows);  // one pass up to 64 rows
    for (int p = 0; wide ? p < jit::wide_passes(rows) : p * 32 < rows; ++p) {
        const JitArgs j = shared_pass_args(ctx, pg, k, rows, p, len, d_srcs, d_dsts);
        KTimer kt(ctx, name, (size_t)blocks);
        RS_HIP(ctx, wide ? launch_rs_jitw(j, blocks, ctx->stream) : launch_rs_jit(j, blocks, ctx->stream));
    }
    return RSGPU_OK;
}

// Host-side handler addresses of coefficient matrix coef[rows][k] in the
// pass layout (rs_kernels.h tc_elem): pass p, source j, slot s -> row 32p + s.
void tc_fill_addr(const rsgpu_ctx* ctx, const uint8_t* coef, int k, int rows, unsigned long long* h)
{
    for (int p = 0; p < tc_passes(rows); ++p) {
        const int pr = tc_pass_rows(rows, p), slots = tc_rows_per_pass(pr);
        unsigned long long* hp = h + tc_pass_offset(k, p);
        for (int j = 0; j < k; ++j)
            for (int s = 0; s < slots; ++s)
                hp[(size_t)j * slots + s] =
                    ctx->h_tc_table[(s & 7) * 256 + (s < pr ? coef[(size_t)(32 * p + s) * k + j] : 0)];
    }
}

// Fill host v_perm tables [k][rows_pad] for coefficient matrix coef[rows][k]
// (coef row r column j at coef[r*k + j]).
void fill_tables(const uint8_t* coef, int k, int rows, int rows_pad, uint4* t4, uint32_t* tc)
{
    for (int j = 0; j < k; ++j)
        for (int r = 0; r < rows_pad; ++r) {
            uint32_t t[5] = {0, 0, 0, 0, 0};
            if (r < rows)
                perm_tables(coef[(size_t)r * k + j], t);
            t4[(size_t)j * rows_pad + r] = make_uint4(t[0], t[1], t[2], t[3]);
            tc[(size_t)j * rows_pad + r] = t[4];
        }
}

// Runtime-coefficient dot product from HOST coefficients coef[rows][k] over
// device pointer tables (d_srcs [blocks][k], d_dsts [blocks][rows]), one
// coefficient table shared by every block, uploaded into scratch at
// tab_off: k_rs_tc for aligned 32-byte-multiple rows, otherwise
// k_dot_generic.  `pre` (pre_bytes <= tab_off, optional) goes to the start
// of scratch in the same upload (the pointer tables of ec_encode_data).
int dot_from_host_coef(rsgpu_ctx* ctx, const uint8_t* coef, int k, int rows, long long len,
                       long long blocks, const uint8_t* const* d_srcs, uint8_t* const* d_dsts,
                       size_t tab_off, bool aligned, const char* tc_name, const char* jit_name,
                       const void* pre = nullptr, size_t pre_bytes = 0)
{
    const bool tcp = aligned && len % 32 == 0 && tc_handlers_ready(ctx);
    if (aligned && len % 32 == 0 && ctx->encode_kernel != RSGPU_ENCODE_THREADED && jit_probe(ctx) == 1) {
        if (pre && pre_bytes <= sizeof(PutArgs::w) && pre_bytes % 8 == 0) {
            // a few row pointers (isa_arithmetic's per-row calls): through the
            // kernel arguments, no staging round trip
            RS_HIP(ctx, launch_put_words(ctx->scratch.p, pre, pre_bytes, ctx->stream));
        } else if (pre) {  // the row pointers the caller staged with the table upload
            void* stage;
            int rc = get_stage(ctx, pre_bytes, &stage);
            if (rc)
                return rc;
            std::memcpy(stage, pre, pre_bytes);
            rc = upload(ctx, ctx->scratch.p, pre_bytes);
            if (rc)
                return rc;
        }
        return shared_program_launch(ctx, coef, k, rows, len, blocks, d_srcs, d_dsts, jit_name);
    }
    const int rows_pad = rows_pad_for(rows);
    const size_t n = (size_t)k * rows_pad;
    const size_t bytes = tcp ? sizeof(unsigned long long) * (size_t)tc_table_elems(k, rows)
                             : n * (sizeof(uint4) + sizeof(uint32_t));
    const size_t skip = pre ? tab_off : 0;  // staging offset of the table
    void* stage;
    int rc = get_stage(ctx, skip + bytes, &stage);
    if (rc)
        return rc;
    if (pre)
        std::memcpy(stage, pre, pre_bytes);
    char* tab = (char*)stage + skip;
    char* d = (char*)ctx->scratch.p + tab_off;
    char* d_up = pre ? (char*)ctx->scratch.p : d;
    if (tcp) {
        tc_fill_addr(ctx, coef, k, rows, (unsigned long long*)tab);
        rc = upload(ctx, d_up, skip + bytes);
        if (rc)
            return rc;
        return tc_launch(ctx, tc_name, d_srcs, d_dsts, (const unsigned long long*)d, 0, k, rows, len,
                         blocks, nullptr);
    }
    uint4* t4 = (uint4*)tab;
    uint32_t* tc = (uint32_t*)(tab + n * sizeof(uint4));
    fill_tables(coef, k, rows, rows_pad, t4, tc);
    rc = upload(ctx, d_up, skip + bytes);
    if (rc)
        return rc;
    DotArgs a{};
    a.srcs = d_srcs;
    a.dsts = d_dsts;
    a.tabs4 = (const uint4*)d;
    a.ctab = (const uint32_t*)(d + n * sizeof(uint4));
    a.tab_block_stride = 0;
    a.k = k;
    a.rows = rows;
    a.rows_pad = rows_pad;
    a.len = len;
    a.blocks = blocks;
    a.status = nullptr;
    a.bytewise = !aligned;
    KTimer kt(ctx, "k_dot_generic", (size_t)blocks);
    RS_HIP(ctx, launch_dot_generic(a, ctx->stream));
    return RSGPU_OK;
}

// scratch bytes dot_from_host_coef needs for its table (either kernel)
size_t dot_table_bytes(int k, int rows)
{
    return std::max(sizeof(unsigned long long) * (size_t)tc_table_elems(k, rows),
                    (size_t)k * rows_pad_for(rows) * (sizeof(uint4) + sizeof(uint32_t)));
}

// AUTO's threshold for the Karatsuba-split (64, 32) encode, in (tile, block)
// pairs per call (profiles/karatsuba3/): the program runs 20 % fewer
// VALU instructions at a lower issue rate, which pays only where the compiled
// kernel runs long enough to sit at the power limit.  C3 (489 x 1024 = 500736
// pairs, a 21 ms encode): step -0.49 ms in every one of 12 ABBA pairs; C4's
// batch (16 x 16384 = 262144, 10.7 ms): level; from 65536 pairs down the
// compiled kernel is 4-30 % faster.
constexpr long long kKaraMinWork = 480000;
// k_rs_kara's chunk rotation period: a chunk is 4 sources of 16 rows per wave
// against k_rs_jitw's 6 (jitw_rot_ticks: 600)
constexpr int kKaraRotTicks = 400;

// The (64, 32) gf_gen_rs_matrix encode through the Karatsuba-split program.
// *unavailable: the program cannot be built in this context (nothing was
// launched, no error is left behind); the context remembers it
// (kara_state) and the caller goes on with the kernels AUTO has otherwise.
int karatsuba_launch(rsgpu_ctx* ctx, long long len, size_t pitch, size_t blocks, const unsigned char* d_src,
                     unsigned char* d_parity, bool* unavailable)
{
    const int k = 64, e = 32;
    *unavailable = false;
    const std::vector<uint8_t> c = parity_matrix(k, e, nullptr);
    int rc = RSGPU_OK;
    const std::string err_before = ctx->err;
    const rsgpu_ctx::SharedProg* pg = shared_program(ctx, c.data(), k, e, &rc, true);
    if (!pg && rc == RSGPU_ERR_UNSUPPORTED) {
        ctx->kara_state = -1;
        ctx->err = err_before;
        *unavailable = true;
        return RSGPU_OK;
    }
    if (!pg)
        return rc;
    RowPtrs rp;
    rc = row_ptr_tables(ctx, k, e, pitch, blocks, d_src, d_parity, rp);
    if (rc)
        return rc;
    JitArgs j = jit_args(rp.src, rp.par, pg->code, pg->chunk_stride, 0, k, e, e, len, nullptr);
    j.chunk_rot_ticks = ctx->jitw_rot >= 0 ? ctx->jitw_rot : kKaraRotTicks;
    j.prio = ctx->jitw_prio;
    KTimer kt(ctx, "k_rs_jit(encode)", blocks);
    RS_HIP(ctx, launch_rs_kara(j, (long long)blocks, ctx->stream));
    return RSGPU_OK;
}

// rsgpu_encode_blocks on at most kMaxGridBlocks blocks, e > 0 and len > 0
int encode_slice(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks, const unsigned char* d_src,
                 unsigned char* d_parity, const unsigned char* coef)
{
    const bool aligned = ptrs_aligned(pitch, d_src, d_parity);
    // The Karatsuba-split generated program of the (64, 32) code (k_rs_kara):
    // KARATSUBA's path wherever it applies, AUTO's from kKaraMinWork (tile,
    // block) pairs; everywhere else KARATSUBA chooses as AUTO.
    const bool kara_wanted = ctx->encode_kernel == RSGPU_ENCODE_KARATSUBA ||
                             (ctx->encode_kernel == RSGPU_ENCODE_AUTO &&
                              (long long)(tiles(len) * blocks) >=
                                  (ctx->kara_min_work >= 0 ? ctx->kara_min_work : kKaraMinWork));
    if (kara_wanted && ctx->kara_state >= 0 && !coef && k == 64 && e == 32 && aligned && len % 32 == 0 &&
        jit_probe(ctx) == 1) {
        bool unavailable;
        const int rc = karatsuba_launch(ctx, (long long)len, pitch, blocks, d_src, d_parity, &unavailable);
        if (!unavailable)
            return rc;
    }
    // Fast paths: the gf_gen_rs_matrix code with compile-time coefficients,
    // bit-sliced (len % 32 == 0) or nibble-table (len % 4 == 0).
    const bool compiled_ok = ctx->encode_kernel == RSGPU_ENCODE_AUTO || ctx->encode_kernel == RSGPU_ENCODE_COMPILED ||
                             ctx->encode_kernel == RSGPU_ENCODE_KARATSUBA;
    if (compiled_ok && !coef && aligned && len % 32 == 0 && rs_bitsliced_split_available(k, e) &&
        (long long)(tiles(len) * blocks) < kTcSplitMaxWork) {
        KTimer kt(ctx, "k_rs_bs_split(encode)", blocks);
        RS_HIP(ctx, launch_rs_bitsliced_split(k, e, d_src, d_parity, (long long)pitch, (long long)len,
                                              (long long)blocks, ctx->stream));
        return RSGPU_OK;
    }
    // AUTO leaves the compiled kernel when its waves own fewer than 8 rows and
    // the two-wave generated layout covers e (16 < e <= 32): (100, 20) builds
    // every source's composites per 5 rows there, per 10 rows in k_rs_jitw --
    // C5 encode 12.8-13.0 vs 14.4 ms (profiles/r03_ab/wide_encode/)
    const bool compiled_pays = ctx->encode_kernel == RSGPU_ENCODE_COMPILED ||
                               rs_bitsliced_rows_per_wave(k, e) >= 8 || !jitw_rows(e) ||
                               !(len % 32 == 0 && jit_probe(ctx) == 1);
    if (compiled_ok && compiled_pays && !coef && aligned && len % 32 == 0 && rs_bitsliced_available(k, e)) {
        KTimer kt(ctx, "k_rs_bs(encode)", blocks);
        RS_HIP(ctx, launch_rs_bitsliced(k, e, d_src, d_parity, (long long)pitch, (long long)len,
                                        (long long)blocks, ctx->stream, ctx->bs_prio));
        return RSGPU_OK;
    }
    if (compiled_ok && !coef && aligned && len % 4 == 0 && len % 32 != 0 &&
        rs_encode_specialized_available(k, e)) {
        KTimer kt(ctx, "k_rs_encode_lh", blocks);
        RS_HIP(ctx, launch_rs_encode_specialized(k, e, d_src, d_parity, (long long)pitch,
                                                 (long long)len, (long long)blocks, ctx->stream));
        return RSGPU_OK;
    }
    const std::vector<uint8_t> c = parity_matrix(k, e, coef);
    RowPtrs rp;
    const int rc = row_ptr_tables(ctx, k, e, pitch, blocks, d_src, d_parity, rp, dot_table_bytes(k, e));
    if (rc)
        return rc;
    return dot_from_host_coef(ctx, c.data(), k, e, (long long)len, (long long)blocks, rp.src, rp.par, rp.bytes,
                              aligned, "k_rs_tc(encode)", "k_rs_jit(encode)");
}

// What the slices of an rsgpu_ec_encode_data_batch call share: the matrix's
// shared program (null: the byte kernel serves every block whole), the v_perm
// tables of the byte kernel in the context's scratch (bytes: it is launched)
// and, behind them, lo [nb] and end [nb] of the slice in flight, which
// k_ec_batch_classify writes and the two kernels read.
struct EcBatch {
    int k, rows, max_len, flags;
    const rsgpu_ctx::SharedProg* pg;
    bool bytes;
    DotArgs dot;
    int* lo;
    int* end;
};

// one slice of at most kMaxGridBlocks blocks: classify, the program over
// [0, lo[b]) in its passes, the byte kernel over [lo[b], end[b])
int ec_batch_slice(rsgpu_ctx* ctx, const EcBatch& c, size_t nb, const uint8_t* const* d_data,
                   uint8_t* const* d_coding, const int* d_len, int* d_status)
{
    {
        const BatchClassifyArgs a{d_data, d_coding, d_len, c.rows ? c.k : 0, c.rows, c.max_len,
                                  c.flags & RSGPU_BATCH_ALIGNED32, c.pg != nullptr, (long long)nb, d_status, c.lo,
                                  c.end};
        KTimer kt(ctx, "classify(ec_batch)", nb);
        RS_HIP(ctx, launch_ec_batch_classify(a, ctx->stream));
    }
    if (c.rows == 0 || c.max_len == 0)
        return RSGPU_OK;
    const long long max_lo = c.max_len & ~31;
    if (c.pg && max_lo > 0) {
        const bool wide = jitw_layout(c.rows);
        for (int p = 0; wide ? p < jit::wide_passes(c.rows) : p * 32 < c.rows; ++p) {
            const JitArgs j = shared_pass_args(ctx, c.pg, c.k, c.rows, p, max_lo, d_data, d_coding);
            KTimer kt(ctx, "k_rs_jit(ec_batch)", nb);
            RS_HIP(ctx, launch_rs_jit_batch(j, wide, c.lo, max_lo, (long long)nb, ctx->stream));
        }
    }
    if (c.bytes) {
        DotArgs a = c.dot;
        a.srcs = d_data;
        a.dsts = d_coding;
        a.blocks = (long long)nb;
        KTimer kt(ctx, "k_dot_bytes(ec_batch)", nb);
        RS_HIP(ctx, launch_dot_bytes_batch(a, c.lo, c.end, ctx->stream));
    }
    return RSGPU_OK;
}

}  // namespace

namespace rsgpu {

int row_ptr_tables(rsgpu_ctx* ctx, int k, int e, size_t pitch, size_t blocks, const uint8_t* d_src,
                   const uint8_t* d_par, RowPtrs& rp, size_t extra)
{
    const size_t src_bytes = align_up(sizeof(void*) * (size_t)k * blocks, 256);
    rp.bytes = src_bytes + align_up(sizeof(void*) * (size_t)e * blocks, 256);
    const int rc = ensure_scratch(ctx, rp.bytes + extra);
    if (rc)
        return rc;
    char* d = (char*)ctx->scratch.p;
    rp.src = (const uint8_t* const*)d;
    rp.par = (uint8_t* const*)(d + src_bytes);
    RS_HIP(ctx, launch_row_ptrs(d_src, (long long)pitch, k, (long long)blocks, (const uint8_t**)d, ctx->stream));
    RS_HIP(ctx, launch_row_ptrs(d_par, (long long)pitch, e, (long long)blocks, (const uint8_t**)(d + src_bytes),
                                ctx->stream));
    return RSGPU_OK;
}

int shared_epilogue_args(rsgpu_ctx* ctx, const uint8_t* coef, int k, int e, long long len, const RowPtrs& rp,
                         JitArgs& j)
{
    int rc = RSGPU_OK;
    const rsgpu_ctx::SharedProg* pg = shared_program(ctx, coef, k, e, &rc);
    if (pg)
        j = shared_pass_args(ctx, pg, k, e, 0, len, rp.src, rp.par);  // e <= 64: one pass
    return rc;
}

const GfTables& host_gf()
{
    static GfTables t = [] {
        GfTables x{};
        gf_build_tables(x);
        return x;
    }();
    return t;
}

uint8_t hmul(uint8_t a, uint8_t b)
{
    const GfTables& t = host_gf();
    return (a && b) ? t.exp[t.log[a] + t.log[b]] : 0;
}

int check_geom(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks)
{
    if (!ctx)
        return RSGPU_ERR_ARG;
    if (k <= 0 || e < 0 || k + e > RSGPU_MAX_SOURCES || pitch < len || blocks == 0)
        return fail(ctx, RSGPU_ERR_ARG, "bad geometry (k, e, len, pitch, blocks)");
    // The kernels that work in 32-byte lanes (rs_bitsliced, rs_jit, rs_tc)
    // load a row's bytes at a 64-bit row base plus a 32-bit offset, the
    // operand of bs::glds32: in a row of 4 GiB or more they would read the
    // sources at off mod 2^32.  (The byte and 16-byte column kernels index
    // in 64 bits; one limit for every path keeps the contract simple.)
    // Pitch and the block count have no such limit.
    if (len > RSGPU_MAX_LEN)
        return fail(ctx, RSGPU_ERR_ARG, "len must be below 4 GiB (at most RSGPU_MAX_LEN)");
    return RSGPU_OK;
}

int ensure_device(rsgpu_ctx* ctx, rsgpu_ctx::DevBuf& b, size_t bytes, size_t floor)
{
    if (b.bytes >= bytes)
        return RSGPU_OK;
    if (b.p) {
        RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        RS_HIP(ctx, hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
    }
    b.key.clear();
    const size_t want = std::max(bytes, floor);
    RS_HIP(ctx, hipMalloc(&b.p, want));
    b.bytes = want;
    return RSGPU_OK;
}

int get_stage(rsgpu_ctx* ctx, size_t bytes, void** out)
{
    if (ctx->stage_pending) {
        RS_HIP(ctx, hipEventSynchronize(ctx->stage_done));
        ctx->stage_pending = false;
    }
    if (ctx->stage_bytes < bytes) {
        if (ctx->h_stage)
            RS_HIP(ctx, hipHostFree(ctx->h_stage));
        size_t want = bytes < (1u << 20) ? (1u << 20) : bytes;
        RS_HIP(ctx, hipHostMalloc(&ctx->h_stage, want));
        ctx->stage_bytes = want;
    }
    *out = ctx->h_stage;
    return RSGPU_OK;
}

int upload(rsgpu_ctx* ctx, void* d_dst, size_t bytes, size_t dst_off, size_t stage_off)
{
    RS_HIP(ctx, hipMemcpyAsync((char*)d_dst + dst_off, (char*)ctx->h_stage + stage_off, bytes,
                               hipMemcpyHostToDevice, ctx->stream));
    RS_HIP(ctx, hipEventRecord(ctx->stage_done, ctx->stream));
    ctx->stage_pending = true;
    return RSGPU_OK;
}

hipEvent_t pool_event(rsgpu_ctx* ctx)
{
    if (!ctx->ev_pool.empty()) {
        hipEvent_t e = ctx->ev_pool.back();
        ctx->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

int ensure_scratch(rsgpu_ctx* ctx, size_t bytes) { return ensure_device(ctx, ctx->scratch, bytes, 1u << 20); }

// Cross-stream ordering events (timing disabled), recycled round-robin: an
// event may be re-recorded once the stream that waits on it has been handed
// the wait, which hipStreamWaitEvent captures at enqueue time.
hipEvent_t sync_event(rsgpu_ctx* ctx)
{
    if (ctx->sync_evs.size() < 32) {
        hipEvent_t e = nullptr;
        (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
        ctx->sync_evs.push_back(e);
        return e;
    }
    hipEvent_t e = ctx->sync_evs[ctx->sync_next];
    ctx->sync_next = (ctx->sync_next + 1) % ctx->sync_evs.size();
    return e;
}

bool tc_handlers_ready(rsgpu_ctx* ctx) { return tc_init(ctx) == 1; }

// The device's coarse-grained pool, found through the owner of a hipMalloc'd
// probe (the HSA agent behind this HIP device): executable allocations for
// the generated decode code come from it.
int jit_probe(rsgpu_ctx* ctx)
{
    if (ctx->jit_state != 0)
        return ctx->jit_state;
    ctx->jit_state = -1;
    void* probe = nullptr;
    if (hipMalloc(&probe, 256) != hipSuccess)
        return -1;
    hsa_amd_pointer_info_t info{};
    info.size = sizeof(info);
    const bool ok = hsa_amd_pointer_info(probe, &info, nullptr, nullptr, nullptr) == HSA_STATUS_SUCCESS;
    (void)hipFree(probe);
    if (!ok)
        return -1;
    hsa_amd_memory_pool_t pool{};
    pool.handle = 0;
    hsa_amd_agent_iterate_memory_pools(info.agentOwner, pick_coarse_pool, &pool);
    if (!pool.handle)
        return -1;
    ctx->jit_pool = pool;
    ctx->jit_state = 1;
    return 1;
}

// >= bytes of executable device memory, filled with returns when (re)made.
// Every kernel that may still execute the old code was enqueued on the
// context stream (or one it waits on): synchronising it retires them.
int jit_ensure(rsgpu_ctx* ctx, size_t bytes)
{
    if (ctx->jit_bytes >= bytes)
        return RSGPU_OK;
    if (jit_probe(ctx) != 1)
        return fail(ctx, RSGPU_ERR_UNSUPPORTED, "no executable device memory pool");
    if (ctx->d_jit) {
        RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        hsa_amd_memory_pool_free(ctx->d_jit);
        ctx->d_jit = nullptr;
        ctx->jit_bytes = 0;
    }
    const size_t want = std::max<size_t>(bytes, 1u << 20);
    void* p = nullptr;
    if (hsa_amd_memory_pool_allocate(ctx->jit_pool, want, HSA_AMD_MEMORY_POOL_EXECUTABLE_FLAG, &p) !=
            HSA_STATUS_SUCCESS || !p)
        return fail(ctx, RSGPU_ERR_NOMEM, "executable device allocation failed");
    ctx->d_jit = p;
    ctx->jit_bytes = want;
    ++ctx->jit_gen;
    RS_HIP(ctx, launch_jit_fill(p, want, ctx->stream));
    return RSGPU_OK;
}

// k_rs_tc over `rows` output rows as passes of <= 32 rows: d_srcs [B][k],
// d_dsts [B][rows] device row-pointer tables, d_addr the pass-layout
// handler addresses, addr_stride elements between blocks' tables (0: one
// table shared by every block).
// Below kTcSplitMaxWork (block, 2 KB tile) pairs a threaded-code pass of <= 8
// rows splits each tile's sources over four waves (k_rs_tc_split): one wave
// per tile leaves most of the 1024 SIMDs idle and walks every source in
// series (C2: one block, 489 tiles)
int tc_launch(rsgpu_ctx* ctx, const char* name, const uint8_t* const* d_srcs, uint8_t* const* d_dsts,
              const unsigned long long* d_addr, long long addr_stride, int k, int rows, long long len,
              long long blocks, const int* d_status)
{
    if (rows <= 8 && k >= 4 && (long long)tiles((size_t)len) * blocks < kTcSplitMaxWork) {
        const TcArgs t = tc_args(d_srcs, d_dsts, rows, d_addr, addr_stride, k, rows, len, d_status);
        KTimer kt(ctx, name, (size_t)blocks);
        RS_HIP(ctx, launch_rs_tc_split(t, blocks, ctx->stream));
        return RSGPU_OK;
    }
    for (int p = 0; p < tc_passes(rows); ++p) {
        const TcArgs t = tc_args(d_srcs, d_dsts + 32 * p, rows, d_addr + tc_pass_offset(k, p), addr_stride, k,
                                 tc_pass_rows(rows, p), len, d_status);
        KTimer kt(ctx, name, (size_t)blocks);
        RS_HIP(ctx, launch_rs_tc(t, blocks, ctx->stream));
    }
    return RSGPU_OK;
}

int rows_pad_for(int rows)
{
    const int R = generic_rows_per_pass(rows);
    return (rows + R - 1) / R * R;
}

std::vector<uint8_t> parity_matrix(int k, int e, const unsigned char* coef)
{
    std::vector<uint8_t> c((size_t)e * k);
    if (coef) {
        std::memcpy(c.data(), coef, c.size());
    } else {
        std::vector<uint8_t> a((size_t)(k + e) * k);
        rsgpu_gf_gen_rs_matrix(a.data(), k + e, k);
        std::memcpy(c.data(), a.data() + (size_t)k * k, c.size());
    }
    return c;
}

}  // namespace rsgpu

extern "C" {

const char* rsgpu_version(void) { return "0.2.0"; }

int rsgpu_create(int device, rsgpu_ctx** out)
{
    if (!out)
        return RSGPU_ERR_ARG;
    *out = nullptr;
    if (hipSetDevice(device) != hipSuccess)
        return RSGPU_ERR_HIP;
    rsgpu_ctx* c = new rsgpu_ctx();
    c->device = device;
    if (hipEventCreateWithFlags(&c->stage_done, hipEventDisableTiming) != hipSuccess) {
        delete c;
        return RSGPU_ERR_HIP;
    }
    *out = c;
    return RSGPU_OK;
}

int rsgpu_destroy(rsgpu_ctx* ctx)
{
    if (!ctx)
        return RSGPU_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (void* p : {ctx->scratch.p, ctx->scrub.p, ctx->d_update, ctx->degraded.p, ctx->rebuild.p,
                    ctx->locate.p})
        if (p)
            (void)hipFree(p);
    if (ctx->h_stage)
        (void)hipHostFree(ctx->h_stage);
    if (ctx->stage_done)
        (void)hipEventDestroy(ctx->stage_done);
    for (auto& r : ctx->recs) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    for (auto e : ctx->ev_pool)
        (void)hipEventDestroy(e);
    for (auto e : ctx->sync_evs)
        (void)hipEventDestroy(e);
    if (ctx->d_tc_table)
        (void)hipFree(ctx->d_tc_table);
    if (ctx->d_jit)
        hsa_amd_memory_pool_free(ctx->d_jit);
    for (auto& pr : ctx->progs)
        hsa_amd_memory_pool_free(pr.code);
    if (ctx->d_code_stage)
        (void)hipFree(ctx->d_code_stage);
    for (hipStream_t st : {ctx->io_in, ctx->io_out, ctx->aux})
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
    if (ctx->d_io)
        (void)hipFree(ctx->d_io);
    for (auto e : ctx->io_evs)
        (void)hipEventDestroy(e);
    delete ctx;
    return RSGPU_OK;
}

int rsgpu_set_stream(rsgpu_ctx* ctx, void* s)
{
    if (!ctx)
        return RSGPU_ERR_ARG;
    hipStream_t ns = (hipStream_t)s;
    if (ns == ctx->stream)
        return RSGPU_OK;
    // everything enqueued on the old stream (kernels reading the scratch
    // tables among them) is ordered before the new stream's work.  The
    // context moves to the new stream even when that cannot be arranged (an
    // old stream already destroyed): it is never left bound to a dead one;
    // the error is reported after the move.
    hipEvent_t ev = sync_event(ctx);
    hipError_t e = hipEventRecord(ev, ctx->stream);
    if (e == hipSuccess)
        e = hipStreamWaitEvent(ns, ev, 0);
    ctx->stream = ns;
    if (e != hipSuccess)
        return fail(ctx, RSGPU_ERR_HIP, std::string("rsgpu_set_stream: ordering against the old stream: ") +
                                            hipGetErrorString(e));
    return RSGPU_OK;
}

void* rsgpu_get_stream(rsgpu_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int rsgpu_synchronize(rsgpu_ctx* ctx)
{
    if (!ctx)
        return RSGPU_ERR_ARG;
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RSGPU_OK;
}

const char* rsgpu_last_error(rsgpu_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int rsgpu_timing_enable(rsgpu_ctx* ctx, int on)
{
    if (!ctx)
        return RSGPU_ERR_ARG;
    ctx->timing = on != 0;
    return RSGPU_OK;
}

int rsgpu_timing_read(rsgpu_ctx* ctx, const char** names, float* ms, size_t* blocks, int max)
{
    if (!ctx || max < 0)
        return RSGPU_ERR_ARG;
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int n = 0;
    for (auto& r : ctx->recs) {
        if (n < max) {
            float t = 0;
            (void)hipEventSynchronize(r.b);  // recorded on an earlier stream, possibly
            (void)hipEventElapsedTime(&t, r.a, r.b);
            if (names)
                names[n] = r.name;
            if (ms)
                ms[n] = t;
            if (blocks)
                blocks[n] = r.blocks;
            ++n;
        }
        ctx->ev_pool.push_back(r.a);
        ctx->ev_pool.push_back(r.b);
    }
    ctx->recs.clear();
    return n;
}

int rsgpu_malloc(rsgpu_ctx* ctx, void** p, size_t bytes)
{
    if (!ctx || !p)
        return RSGPU_ERR_ARG;
    if (hipMalloc(p, bytes ? bytes : 1) != hipSuccess)
        return fail(ctx, RSGPU_ERR_NOMEM, "hipMalloc failed");
    return RSGPU_OK;
}

int rsgpu_free(rsgpu_ctx* ctx, void* p)
{
    if (!ctx)
        return RSGPU_ERR_ARG;
    RS_HIP(ctx, hipFree(p));
    return RSGPU_OK;
}

int rsgpu_memcpy_h2d(rsgpu_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (!ctx)
        return RSGPU_ERR_ARG;
    RS_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RSGPU_OK;
}

int rsgpu_memcpy_d2h(rsgpu_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (!ctx)
        return RSGPU_ERR_ARG;
    RS_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RSGPU_OK;
}

// ---- host GF helpers -------------------------------------------------------

unsigned char rsgpu_gf_mul(unsigned char a, unsigned char b) { return hmul(a, b); }

unsigned char rsgpu_gf_inv(unsigned char a)
{
    const GfTables& t = host_gf();
    return a ? t.exp[255 - t.log[a]] : 0;
}

void rsgpu_gf_gen_rs_matrix(unsigned char* a, int m, int k)
{
    std::memset(a, 0, (size_t)m * k);
    for (int i = 0; i < k; ++i)
        a[(size_t)k * i + i] = 1;
    uint8_t gen = 1;
    for (int i = k; i < m; ++i) {
        uint8_t p = 1;
        for (int j = 0; j < k; ++j) {
            a[(size_t)k * i + j] = p;
            p = hmul(p, gen);
        }
        gen = hmul(gen, 2);
    }
}

void rsgpu_gf_gen_cauchy1_matrix(unsigned char* a, int m, int k)
{
    std::memset(a, 0, (size_t)m * k);
    for (int i = 0; i < k; ++i)
        a[(size_t)k * i + i] = 1;
    unsigned char* p = a + (size_t)k * k;
    for (int i = k; i < m; ++i)
        for (int j = 0; j < k; ++j)
            *p++ = rsgpu_gf_inv((unsigned char)(i ^ j));
}

int rsgpu_gf_invert_matrix(unsigned char* in, unsigned char* out, const int n)
{
    std::memset(out, 0, (size_t)n * n);
    for (int i = 0; i < n; ++i)
        out[(size_t)i * n + i] = 1;
    for (int i = 0; i < n; ++i) {
        if (in[(size_t)i * n + i] == 0) {
            int j = i + 1;
            while (j < n && in[(size_t)j * n + i] == 0)
                ++j;
            if (j == n)
                return -1;
            for (int c = 0; c < n; ++c) {
                std::swap(in[(size_t)i * n + c], in[(size_t)j * n + c]);
                std::swap(out[(size_t)i * n + c], out[(size_t)j * n + c]);
            }
        }
        const uint8_t piv = rsgpu_gf_inv(in[(size_t)i * n + i]);
        for (int c = 0; c < n; ++c) {
            in[(size_t)i * n + c] = hmul(in[(size_t)i * n + c], piv);
            out[(size_t)i * n + c] = hmul(out[(size_t)i * n + c], piv);
        }
        for (int r = 0; r < n; ++r) {
            if (r == i)
                continue;
            const uint8_t f = in[(size_t)r * n + i];
            if (!f)
                continue;
            for (int c = 0; c < n; ++c) {
                out[(size_t)r * n + c] ^= hmul(f, out[(size_t)i * n + c]);
                in[(size_t)r * n + c] ^= hmul(f, in[(size_t)i * n + c]);
            }
        }
    }
    return 0;
}

void rsgpu_gf_vect_mul_init(unsigned char c, unsigned char* tbl)
{
    for (int x = 0; x < 16; ++x) {
        tbl[x] = hmul(c, (uint8_t)x);
        tbl[16 + x] = hmul(c, (uint8_t)(x << 4));
    }
}

void rsgpu_ec_init_tables(int k, int rows, unsigned char* a, unsigned char* g)
{
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < k; ++j) {
            rsgpu_gf_vect_mul_init(*a++, g);
            g += 32;
        }
}

// ---- device, ISA-L-shaped ----------------------------------------------------

int rsgpu_ec_encode_data(rsgpu_ctx* ctx, int len, int k, int rows, const unsigned char* gftbls,
                         unsigned char** data, unsigned char** coding)
{
    if (!ctx || len < 0 || k <= 0 || rows < 0 || k > RSGPU_MAX_SOURCES || rows > 255 ||
        (rows > 0 && (!gftbls || !data || !coding)))
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_ec_encode_data: bad arguments");
    if (rows == 0 || len == 0)
        return RSGPU_OK;
    // coefficient = tbl[1] of each 32-byte table (isa/ec_base.c:300)
    std::vector<uint8_t> coef((size_t)rows * k);
    for (int r = 0; r < rows; ++r)
        for (int j = 0; j < k; ++j)
            coef[(size_t)r * k + j] = gftbls[((size_t)r * k + j) * 32 + 1];
    bool aligned = true;
    for (int j = 0; j < k; ++j)
        aligned &= ((uintptr_t)data[j] & 15) == 0;
    for (int r = 0; r < rows; ++r)
        aligned &= ((uintptr_t)coding[r] & 15) == 0;
    const size_t ptr_bytes = align_up(sizeof(void*) * (size_t)(k + rows), 256);
    int rc = ensure_scratch(ctx, ptr_bytes + dot_table_bytes(k, rows));
    if (rc)
        return rc;
    // the row pointers go up in the same upload as the coefficient table
    std::vector<void*> hp((size_t)(k + rows));
    for (int j = 0; j < k; ++j)
        hp[j] = data[j];
    for (int r = 0; r < rows; ++r)
        hp[k + r] = coding[r];
    char* d = (char*)ctx->scratch.p;
    return dot_from_host_coef(ctx, coef.data(), k, rows, len, 1, (const uint8_t* const*)d,
                              (uint8_t* const*)(d + sizeof(void*) * k), ptr_bytes, aligned,
                              "k_rs_tc(ec_encode_data)", "k_rs_jit(ec_encode_data)", hp.data(),
                              sizeof(void*) * hp.size());
}

int rsgpu_ec_encode_data_batch(rsgpu_ctx* ctx, int k, int rows, const unsigned char* gftbls, size_t blocks,
                               const unsigned char* const* d_data, unsigned char* const* d_coding,
                               const int* d_len, int max_len, int flags, int* d_status)
{
    if (!ctx || !ec_batch_args_ok(k, rows, gftbls && d_data && d_coding && d_len, max_len, flags))
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_ec_encode_data_batch: bad arguments");
    if (blocks == 0)
        return RSGPU_OK;
    if (!d_len) {  // rows == 0 and nothing to judge
        if (d_status)
            RS_HIP(ctx, hipMemsetAsync(d_status, 0, sizeof(int) * blocks, ctx->stream));
        return RSGPU_OK;
    }
    const bool work = rows > 0 && max_len > 0;
    if (!work && !d_status)
        return RSGPU_OK;
    EcBatch c{};
    c.k = k;
    c.rows = rows;
    c.max_len = max_len;
    c.flags = flags;
    std::vector<uint8_t> coef((size_t)rows * k);
    if (work) {
        // coefficient = tbl[1] of each 32-byte table, as rsgpu_ec_encode_data
        for (size_t i = 0; i < coef.size(); ++i)
            coef[i] = gftbls[i * 32 + 1];
        if (ctx->encode_kernel != RSGPU_ENCODE_THREADED && jit_probe(ctx) == 1) {
            int rc = RSGPU_OK;
            const std::string err_before = ctx->err;
            c.pg = shared_program(ctx, coef.data(), k, rows, &rc);
            if (!c.pg && rc != RSGPU_ERR_UNSUPPORTED)
                return rc;
            if (!c.pg)
                ctx->err = err_before;  // the byte kernel serves: no error is left behind
        }
        c.bytes = !c.pg || !(flags & RSGPU_BATCH_ALIGNED32);
    }
    const size_t nb_max = std::min(blocks, kMaxGridBlocks);
    const size_t tab_bytes = c.bytes ? align_up(dot_table_bytes(k, rows), 256) : 0;
    int rc = ensure_scratch(ctx, tab_bytes + 2 * sizeof(int) * nb_max);
    if (rc)
        return rc;
    char* d = (char*)ctx->scratch.p;
    c.lo = (int*)(d + tab_bytes);
    c.end = c.lo + nb_max;
    if (c.bytes) {
        const int rows_pad = rows_pad_for(rows);
        const size_t n = (size_t)k * rows_pad;
        void* stage;
        rc = get_stage(ctx, n * (sizeof(uint4) + sizeof(uint32_t)), &stage);
        if (rc)
            return rc;
        fill_tables(coef.data(), k, rows, rows_pad, (uint4*)stage, (uint32_t*)((char*)stage + n * sizeof(uint4)));
        rc = upload(ctx, d, n * (sizeof(uint4) + sizeof(uint32_t)));
        if (rc)
            return rc;
        c.dot.tabs4 = (const uint4*)d;
        c.dot.ctab = (const uint32_t*)(d + n * sizeof(uint4));
        c.dot.tab_block_stride = 0;
        c.dot.k = k;
        c.dot.rows = rows;
        c.dot.rows_pad = rows_pad;
        c.dot.len = max_len;
    }
    return for_grid_slices(blocks, [&](size_t b0, size_t nb) {
        return ec_batch_slice(ctx, c, nb, d_data ? d_data + b0 * k : nullptr, d_coding ? d_coding + b0 * rows : nullptr,
                              d_len + b0, d_status ? d_status + b0 : nullptr);
    });
}

int rsgpu_ec_encode_data_update(rsgpu_ctx* ctx, int len, int k, int rows, int vec_i,
                                const unsigned char* gftbls, unsigned char* data,
                                unsigned char** coding)
{
    if (!ctx || len < 0 || k <= 0 || rows < 0 || vec_i < 0 || vec_i >= k || rows > 255 ||
        (rows > 0 && (!gftbls || !data || !coding)))
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_ec_encode_data_update: bad arguments");
    if (rows == 0 || len == 0)
        return RSGPU_OK;
    const size_t ptr_bytes = align_up(sizeof(void*) * (size_t)rows, 256);
    const size_t tab_bytes = (size_t)rows * (sizeof(uint4) + sizeof(uint32_t));
    int rc = ensure_scratch(ctx, ptr_bytes + tab_bytes);
    if (rc)
        return rc;
    void* stage;
    rc = get_stage(ctx, ptr_bytes + tab_bytes, &stage);
    if (rc)
        return rc;
    void** hp = (void**)stage;
    for (int r = 0; r < rows; ++r)
        hp[r] = coding[r];
    uint4* t4 = (uint4*)((char*)stage + ptr_bytes);
    uint32_t* tc = (uint32_t*)((char*)t4 + (size_t)rows * sizeof(uint4));
    for (int r = 0; r < rows; ++r) {
        uint32_t t[5];
        // coefficient of (row r, column vec_i): tbl[1] (isa/ec_base.c:316)
        perm_tables(gftbls[((size_t)r * k + vec_i) * 32 + 1], t);
        t4[r] = make_uint4(t[0], t[1], t[2], t[3]);
        tc[r] = t[4];
    }
    rc = upload(ctx, ctx->scratch.p, ptr_bytes + tab_bytes);
    if (rc)
        return rc;
    char* d = (char*)ctx->scratch.p;
    RS_HIP(ctx, launch_update(data, (uint8_t* const*)d, (const uint4*)(d + ptr_bytes),
                              (const uint32_t*)(d + ptr_bytes + (size_t)rows * sizeof(uint4)),
                              rows, len, ctx->stream));
    return RSGPU_OK;
}

int rsgpu_gf_vect_dot_prod(rsgpu_ctx* ctx, int len, int vlen, const unsigned char* gftbls, unsigned char** src,
                           unsigned char* dest)
{
    if (!ctx || len < 0 || vlen <= 0 || !gftbls || !src || !dest)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_gf_vect_dot_prod: bad arguments");
    unsigned char* coding[1] = {dest};
    return rsgpu_ec_encode_data(ctx, len, vlen, 1, gftbls, src, coding);
}

int rsgpu_gf_vect_mad(rsgpu_ctx* ctx, int len, int vec, int vec_i, const unsigned char* gftbls, unsigned char* src,
                      unsigned char* dest)
{
    if (!ctx || len < 0 || vec <= 0 || vec_i < 0 || vec_i >= vec || !gftbls || !src || !dest)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_gf_vect_mad: bad arguments");
    unsigned char* coding[1] = {dest};
    return rsgpu_ec_encode_data_update(ctx, len, vec, 1, vec_i, gftbls, src, coding);
}

int rsgpu_gf_vect_mul(rsgpu_ctx* ctx, int len, const unsigned char* gftbl, void* src, void* dest)
{
    if (!ctx || len < 0 || len % 32 != 0 || !gftbl || !src || !dest)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_gf_vect_mul: len must be a multiple of 32 (gf_vect_mul.h:96-101)");
    unsigned char* data[1] = {(unsigned char*)src};
    unsigned char* coding[1] = {(unsigned char*)dest};
    return rsgpu_ec_encode_data(ctx, len, 1, 1, gftbl, data, coding);
}

// ---- device, batched -----------------------------------------------------------

int rsgpu_encode_blocks(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                        const unsigned char* d_src, unsigned char* d_parity,
                        const unsigned char* coef)
{
    int rc = check_geom(ctx, k, e, len, pitch, blocks);
    if (rc)
        return rc;
    if (e == 0 || len == 0)
        return RSGPU_OK;
    return for_grid_slices(blocks, [&](size_t b0, size_t nb) {
        return encode_slice(ctx, k, e, len, pitch, nb, d_src + b0 * k * pitch, d_parity + b0 * e * pitch, coef);
    });
}

int rsgpu_set_encode_kernel(rsgpu_ctx* ctx, int kernel)
{
    if (!ctx || kernel < RSGPU_ENCODE_AUTO || kernel > RSGPU_ENCODE_KARATSUBA)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_set_encode_kernel: unknown kernel");
    ctx->encode_kernel = kernel;
    return RSGPU_OK;
}

int rsgpu_fill_synthetic(rsgpu_ctx* ctx, unsigned char* d_rows, size_t rows, size_t len,
                         size_t pitch, uint64_t seed, uint64_t row0)
{
    if (!ctx || pitch < len)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_fill_synthetic: bad arguments");
    if (rows == 0 || len == 0)
        return RSGPU_OK;
    RS_HIP(ctx, launch_fill_synth(d_rows, (long long)rows, (long long)len, (long long)pitch, seed,
                                  row0, ctx->stream));
    return RSGPU_OK;
}

int rsgpu_erasure_patterns(uint64_t seed, uint64_t blk0, size_t blocks, int k, int e,
                           unsigned char* h_err)
{
    if (!h_err || k <= 0 || e < 0 || e > k || k > 256)
        return RSGPU_ERR_ARG;
    for (size_t b = 0; b < blocks; ++b)
        erasure_pattern(seed, blk0 + b, k, e, h_err + b * (size_t)e);
    return RSGPU_OK;
}

}  // extern "C"
