// rsgpu_testhooks.cpp -- test and A/B hooks, built into their OWN library
// (rsgpu/librsgpu_testhooks.so), never into librsgpu.so, whose exports are
// exactly include/rsgpu.h (rsgpu.map).  The CPU suite interprets the code
// the host emitters write (tests/test_jit.py), the GPU suite compares the
// device emitter with them and drives the generated decode's layout knobs,
// and tools/ab_lib.py uses the knobs for same-box A/Bs.  The context hooks
// write fields of an rsgpu_ctx created by librsgpu.so (the struct is
// rsgpu_ctx.h, compiled into both); the emitters link their own copies of
// jit_prog.o and rs_jit.o.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/rsgpu.h"
#include "jit_prog.h"
#include "plane_mul.h"
#include "rs_jit.h"
#include "rs_kernels.h"
#include "rs_lane.h"
#include "rs_pairs.h"
#include "rsgpu_ctx.h"
#include "rsgpu_internal.h"

using namespace rsgpu;

namespace {

// One pass's code in the two- / four-wave layout (rs_jit.h Wide<R, CS>):
// rows row_base .. row_base + rows - 1 of the e x k matrix coef, from
// Wide::code_word: wave w, chunk ch at (w nch + ch) chunk_stride from o64;
// unused words are returns.
template <class W>
void jitw_emit_host(int k, int row_base, int rows, const unsigned char* coef, uint64_t* o64)
{
    const int nch = (k + W::CS - 1) / W::CS, stride_w = W::chunk_stride() / 8;
    for (int w = 0; w < jit::wide_waves(rows); ++w) {
        const int r0 = row_base + jit::wide_row0(rows, w);
        const int nslot = jit::wide_row0(rows, w + 1) - jit::wide_row0(rows, w);
        const unsigned char* cr = coef + (size_t)r0 * k;
        for (int ch = 0; ch < nch; ++ch)
            for (int o = 0; o < stride_w; ++o) {
                uint64_t word;
                if (W::code_word(cr, k, nslot, ch, o, &word))
                    o64[((size_t)w * nch + ch) * stride_w + o] = word;
            }
    }
}

}  // namespace

extern "C" {

// Test / A-B hook (not part of include/rsgpu.h): column tiles per workgroup
// of the two-wave generated decode (1, 2, 3; 0 = the library's choice).
int rsgpu_internal_set_jitw_tiles(rsgpu_ctx* ctx, int n)
{
    if (!ctx || n < 0 || n > 3)
        return RSGPU_ERR_ARG;
    ctx->jitw_tpw = n;
    return RSGPU_OK;
}

// A-B hook (not part of include/rsgpu.h): k_rs_jitw's code prefetch into L2
// (0 off, 1 on, -1 the library's choice).
int rsgpu_internal_set_jitw_prefetch(rsgpu_ctx* ctx, int n)
{
    if (!ctx || n < -1 || n > 1)
        return RSGPU_ERR_ARG;
    ctx->jitw_prefetch = n;
    return RSGPU_OK;
}

// A-B hook (not part of include/rsgpu.h): k_rs_jitw's chunk rotation period
// in 100 MHz ticks (0 chunks in order, -1 the library's choice).
int rsgpu_internal_set_jitw_rot(rsgpu_ctx* ctx, int n)
{
    if (!ctx || n < -1 || n > 1000000)
        return RSGPU_ERR_ARG;
    ctx->jitw_rot = n;
    return RSGPU_OK;
}

// A-B hook (not part of include/rsgpu.h): the generated-code kernels
// (k_rs_jitw, k_rs_jit) raise their waves' priority (to level 2) from the
// transposes to the chunk barrier (n != 0, the default 2) or not (0).
int rsgpu_internal_set_jitw_prio(rsgpu_ctx* ctx, int n)
{
    if (!ctx || n < 0 || n > 3)
        return RSGPU_ERR_ARG;
    ctx->jitw_prio = n;
    return RSGPU_OK;
}

// A-B hook (not part of include/rsgpu.h): k_rs_bs raises its waves'
// priority (to level 2) from the transposes to the part barrier (n != 0, the
// default 2; its own instantiation) or not (0).
int rsgpu_internal_set_bs_prio(rsgpu_ctx* ctx, int n)
{
    if (!ctx || n < 0 || n > 3)
        return RSGPU_ERR_ARG;
    ctx->bs_prio = n;
    return RSGPU_OK;
}

// Test / A-B hook (not part of include/rsgpu.h): slices of the short-row
// generated decode whose prepare and emission run beside the decode
// (rsgpu_decode_blocks; 0 or 1 off, -1 the library's choice).
int rsgpu_internal_set_decode_pipeline(rsgpu_ctx* ctx, int n)
{
    if (!ctx || n < -1 || n > 64)
        return RSGPU_ERR_ARG;
    ctx->decode_pipe = n;
    return RSGPU_OK;
}

// Test hooks (not part of include/rsgpu.h) of the rebuild of long lists
// (rsgpu_scrub.cpp rebuild_wide).  k_rs_tc jumps to the addresses
// k_rebuild_wide_prepare writes, so the GPU suite looks at them before the
// first launch: with prepare_only set, rsgpu_rebuild_blocks stops after the
// wide prepare (reports written, no row touched); rebuild_wide_layout then
// tells where the last group's tables lie in the context's buffer --
// out[0..9] = blocks of a group, k, passes, slots, bytes between blocks' lane
// tables, and the offsets of the lane tables, handler addresses [B][k][slots],
// source pointers [B][k], destination pointers [B][slots] and counts [B] --
// rebuild_wide_read copies bytes of that buffer to the host, and tc_table
// gives the context's 2048 handler addresses [slot & 7][coefficient] (-1
// before the first call that needed them).  rebuild_group caps the blocks of a
// group (0: the 64 MiB rule), so that a small call runs as several groups.
int rsgpu_internal_set_rebuild_prepare_only(rsgpu_ctx* ctx, int on)
{
    if (!ctx)
        return RSGPU_ERR_ARG;
    ctx->rebuild_prepare_only = on != 0;
    return RSGPU_OK;
}

int rsgpu_internal_set_rebuild_group(rsgpu_ctx* ctx, long long blocks)
{
    if (!ctx || blocks < 0)
        return RSGPU_ERR_ARG;
    ctx->rebuild_group_max = (size_t)blocks;
    return RSGPU_OK;
}

// Test hook (not part of include/rsgpu.h): caps the blocks of a group of
// rsgpu_locate_blocks (0: the 64 MiB rule), so that a small call runs as
// several groups.
int rsgpu_internal_set_locate_group(rsgpu_ctx* ctx, long long blocks)
{
    if (!ctx || blocks < 0)
        return RSGPU_ERR_ARG;
    ctx->locate_group_max = (size_t)blocks;
    return RSGPU_OK;
}

// Test hook (not part of include/rsgpu.h): caps the blocks of a group of
// rsgpu_scrub_degraded_blocks (0: the 64 MiB rule), so that a small call runs
// as several groups.
int rsgpu_internal_set_degraded_group(rsgpu_ctx* ctx, long long blocks)
{
    if (!ctx || blocks < 0)
        return RSGPU_ERR_ARG;
    ctx->degraded_group_max = (size_t)blocks;
    return RSGPU_OK;
}

// Test hook (not part of include/rsgpu.h): the bytes of the scrub family's
// device buffer [tables | parity scratch of the two-pass forms] as the context
// holds it now, 0 before the first call that needed it -- for the tests of the
// forms that must not grow it.
long long rsgpu_internal_scrub_scratch_bytes(rsgpu_ctx* ctx)
{
    return ctx ? (long long)ctx->scrub.bytes : (long long)RSGPU_ERR_ARG;
}

int rsgpu_internal_rebuild_wide_layout(rsgpu_ctx* ctx, long long* out)
{
    if (!ctx || !out || ctx->rebuild_wide.blocks == 0)
        return RSGPU_ERR_ARG;
    const rsgpu_ctx::RebuildWideLayout& l = ctx->rebuild_wide;
    const long long v[10] = {(long long)l.blocks, l.k, l.passes, l.slots, (long long)l.lane_stride,
                             (long long)l.lane, (long long)l.addr, (long long)l.srcs, (long long)l.dsts,
                             (long long)l.count};
    std::memcpy(out, v, sizeof v);
    return RSGPU_OK;
}

int rsgpu_internal_rebuild_wide_read(rsgpu_ctx* ctx, size_t offset, void* out, size_t bytes)
{
    if (!ctx || !out || !ctx->rebuild.p || offset > ctx->rebuild.bytes || bytes > ctx->rebuild.bytes - offset)
        return RSGPU_ERR_ARG;
    if (hipMemcpyAsync(out, (const char*)ctx->rebuild.p + offset, bytes, hipMemcpyDeviceToHost, ctx->stream) !=
            hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
        return RSGPU_ERR_HIP;
    return RSGPU_OK;
}

int rsgpu_internal_tc_table(rsgpu_ctx* ctx, unsigned long long* out)
{
    if (!ctx || !out || ctx->tc_state != 1)
        return RSGPU_ERR_ARG;
    std::memcpy(out, ctx->h_tc_table, sizeof ctx->h_tc_table);
    return RSGPU_OK;
}

// Test hook (not in include/rsgpu.h): the host-built code of an e x k matrix
// shared by every block (jit_prog.h, the GENERATED encode), for the CPU
// suite to disassemble and interpret.  Returns the bytes needed, or -1;
// writes only when out_bytes is large enough; *chunk_stride gets the stride.
long long rsgpu_internal_jit_matrix_code(int k, int e, const unsigned char* coef, unsigned char* out,
                                         size_t out_bytes, int* chunk_stride, int max_ops)
{
    if (k <= 0 || k > 250 || e <= 0 || e > 255 || !coef || !chunk_stride)
        return -1;
    const std::vector<uint8_t> code = jit::build_matrix_code(coef, k, e, chunk_stride, max_ops);
    if (out && out_bytes >= code.size())
        std::memcpy(out, code.data(), code.size());
    return (long long)code.size();
}

// Test hook (not part of include/rsgpu.h): the generated decode code of ONE
// block for coefficient matrix coef[e][k], written on the host by the same
// emitters the prepare kernel runs (rs_jit.h), so the CPU suite can
// disassemble and interpret it.  Returns the bytes needed (jit_code_bytes)
// or -1 for bad arguments; writes only when out_bytes is large enough.
long long rsgpu_internal_jit_emit(int k, int e, const unsigned char* coef, unsigned char* out,
                                  size_t out_bytes)
{
    if (k <= 0 || e <= 0 || k + e > 250 || !coef)
        return -1;
    const size_t need = jit_code_bytes(k, e, 1);
    if (!out || out_bytes < need)
        return (long long)need;
    const int nw = (e + 7) / 8, nch = (k + 7) / 8, stride_w = jit::chunk_stride(8) / 8;
    uint64_t* o64 = reinterpret_cast<uint64_t*>(out);
    for (size_t i = 0; i < need / 8; ++i)
        o64[i] = (uint64_t)jit::S_NOP0 << 32 | jit::S_SETPC_82;
    // the words k_jit_emit writes, from the same function
    for (int w = 0; w < nw; ++w) {
        const int nslot = std::min(8, e - 8 * w);
        const unsigned char* rows = coef + (size_t)8 * w * k;
        for (int ch = 0; ch < nch; ++ch)
            for (int o = 0; o < stride_w; ++o) {
                uint64_t word;
                if (jit::code_word(rows, k, nslot, ch, o, &word))
                    o64[((size_t)w * nch + ch) * stride_w + o] = word;
            }
    }
    return (long long)need;
}

// Test hook (not part of include/rsgpu.h): the same for the two- and
// four-wave layouts of k_rs_jitw (rs_jit.h Wide, jitw_rows, wide_waves; e >
// 64 as passes of <= 64 rows, wide_passes), from Wide::code_word (the words
// k_jitw_emit writes).
long long rsgpu_internal_jitw_emit(int k, int e, const unsigned char* coef, unsigned char* out,
                                   size_t out_bytes)
{
    if (k <= 0 || !jitw_layout(e) || k + e > 250 || !coef)
        return -1;
    const size_t need = jitw_code_bytes(k, e, 1);
    if (!out || out_bytes < need)
        return (long long)need;
    uint64_t* o64 = reinterpret_cast<uint64_t*>(out);
    for (size_t i = 0; i < need / 8; ++i)
        o64[i] = (uint64_t)jit::S_NOP0 << 32 | jit::S_SETPC_82;
    for (int p = 0; p < jit::wide_passes(e); ++p) {  // passes of <= 64 rows (e > 64)
        const int r0 = jit::wide_pass_row0(e, p), rows = jit::wide_pass_rows(e, p);
        uint64_t* po = o64 + jitw_pass_offset(k, e, p) / 8;
        if (jitw_rows(rows) == 16)
            jitw_emit_host<jit::J16>(k, r0, rows, coef, po);
        else if (jitw_rows(rows) == 12)
            jitw_emit_host<jit::J12>(k, r0, rows, coef, po);
        else
            jitw_emit_host<jit::J10>(k, r0, rows, coef, po);
    }
    return (long long)need;
}

// Test hook (not in include/rsgpu.h): the host-built shared program of an
// e x k matrix in the two- or four-wave layout (16 < e <= 125; passes of <= 64
// rows above 64), built exactly as shared_program builds it, for the CPU suite
// to disassemble and interpret.  Returns the bytes needed, or -1; writes only
// when out_bytes is large enough; pass p's byte offset and chunk stride go to
// pass_off[p] / pass_stride[p] (p < max_passes), *npasses gets the count.
long long rsgpu_internal_jitw_matrix_code(int k, int e, const unsigned char* coef, unsigned char* out,
                                          size_t out_bytes, long long* pass_off, int* pass_stride, int max_passes,
                                          int* npasses, int max_ops)
{
    if (k <= 0 || k + e > 250 || !jitw_layout(e) || !coef || !pass_off || !pass_stride || !npasses)
        return -1;
    std::vector<std::pair<size_t, int>> passes;
    const std::vector<uint8_t> code = jit::build_matrix_code_wide_passes(coef, k, e, &passes, max_ops);
    if (code.empty() || (int)passes.size() > max_passes)
        return -1;
    *npasses = (int)passes.size();
    for (size_t p = 0; p < passes.size(); ++p) {
        pass_off[p] = (long long)passes[p].first;
        pass_stride[p] = passes[p].second;
    }
    if (out && out_bytes >= code.size())
        std::memcpy(out, code.data(), code.size());
    return (long long)code.size();
}

// Test hook (not in include/rsgpu.h): the Karatsuba-split program of the
// (64, 32) code with parity matrix coef [32][64] (jit_prog.h
// build_karatsuba_code), as shared_program builds it: the code (role w, chunk
// ch at (w 9 + ch) *chunk_stride), and the role matrices cP / cQ1 / cQ2
// [16][32], rho [32] and sigma [16] into mats (1584 bytes, in that order).
// Returns the code bytes, or -1 (coef is not the gf_gen_rs_matrix code).
long long rsgpu_internal_jit_karatsuba_code(const unsigned char* coef, unsigned char* out, size_t out_bytes,
                                            int* chunk_stride, unsigned char* mats)
{
    jit::KaraProgram kp;
    if (!coef || !chunk_stride || !jit::build_karatsuba_code(coef, &kp))
        return -1;
    *chunk_stride = kp.chunk_stride;
    if (mats) {
        std::memcpy(mats, kp.cP, 512);
        std::memcpy(mats + 512, kp.cQ1, 512);
        std::memcpy(mats + 1024, kp.cQ2, 512);
        std::memcpy(mats + 1536, kp.rho, 32);
        std::memcpy(mats + 1568, kp.sigma, 16);
    }
    if (out && out_bytes >= kp.code.size())
        std::memcpy(out, kp.code.data(), kp.code.size());
    return (long long)kp.code.size();
}

// Test / A-B hook (not part of include/rsgpu.h): the (tile, block) pairs from
// which AUTO encodes (64, 32) through the Karatsuba program (-1 = the
// library's threshold).
int rsgpu_internal_set_kara_min_work(rsgpu_ctx* ctx, long long pairs)
{
    if (!ctx || pairs < -1)
        return RSGPU_ERR_ARG;
    ctx->kara_min_work = pairs;
    return RSGPU_OK;
}

// Test hook (not part of include/rsgpu.h): mark the Karatsuba program as
// not buildable in this context (-1), as a failed build leaves it, or clear
// that (0).
int rsgpu_internal_set_kara_state(rsgpu_ctx* ctx, int state)
{
    if (!ctx || (state != 0 && state != -1))
        return RSGPU_ERR_ARG;
    ctx->kara_state = state;
    return RSGPU_OK;
}

// Test hook (not part of include/rsgpu.h): the DEVICE emitter k_jitw_emit
// for `blocks` blocks of decode rows coef [blocks][e][k] (host memory), its
// code copied back into out (blocks x the bytes rsgpu_internal_jitw_emit
// returns for one block), so a GPU test compares it word for word with the
// host emitter the CPU suite interprets.  Returns the bytes, or -1.
long long rsgpu_internal_jitw_emit_device(rsgpu_ctx* ctx, int k, int e, size_t blocks,
                                          const unsigned char* coef, unsigned char* out, size_t out_bytes)
{
    if (!ctx || k <= 0 || !jitw_layout(e) || k + e > 250 || blocks == 0 || blocks > kMaxGridBlocks || !coef)
        return -1;
    const size_t need = jitw_code_bytes(k, e, (long long)blocks);
    if (!out || out_bytes < need)
        return (long long)need;
    uint8_t *d_coef = nullptr, *d_code = nullptr;
    int* d_status = nullptr;
    long long rc = -1;
    if (hipMalloc(&d_coef, blocks * e * k) == hipSuccess && hipMalloc(&d_code, need) == hipSuccess &&
        hipMalloc(&d_status, blocks * sizeof(int)) == hipSuccess &&
        hipMemcpyAsync(d_coef, coef, blocks * e * k, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
        hipMemsetAsync(d_status, 0, blocks * sizeof(int), ctx->stream) == hipSuccess &&
        launch_jit_fill(d_code, need, ctx->stream) == hipSuccess &&
        launch_jitw_emit(k, e, (long long)blocks, d_coef, d_status, d_code, ctx->stream) == hipSuccess &&
        hipMemcpyAsync(out, d_code, need, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
        hipStreamSynchronize(ctx->stream) == hipSuccess)
        rc = (long long)need;
    (void)hipFree(d_coef);
    (void)hipFree(d_code);
    (void)hipFree(d_status);
    return rc;
}

// Test hook (not part of include/rsgpu.h): the scrub kernels' location rule
// (rs_lane.h scrub_locate_row) on the host, for the CPU suite to compare with
// the model's brute force: the row that explains the syndrome column syn [e]
// (not all zero) under the e x k matrix coef and its ratio -> row table
// rowtab [256] (255: none), or -1.
int rsgpu_internal_scrub_locate_row(int k, int e, const unsigned char* rowtab, const unsigned char* coef,
                                    const unsigned char* syn)
{
    static const GfTables gf = make_gf_tables();
    int nz = 0, p0 = 0;
    for (int p = 0; p < e; ++p)
        if (syn[p]) {
            ++nz;
            p0 = p;
        }
    if (!nz || e < 2)
        return -1;
    return scrub_locate_row(k, e, rowtab, coef, gf, syn[0], syn[1], nz, p0, [&](int p) { return syn[p]; });
}

// Test hook (not part of include/rsgpu.h): the constant-times-planes multiply
// of k_rs_bs_degraded's reduction (plane_mul.h) on the host: t[0..7] ^= c * s
// [0..7], plane a holding bit a of 32 bytes.
int rsgpu_internal_plane_mul_acc(unsigned c, const uint32_t* s, uint32_t* t)
{
    if (c > 255 || !s || !t)
        return RSGPU_ERR_ARG;
    uint32_t sv[8], tv[8];
    std::memcpy(sv, s, sizeof sv);
    std::memcpy(tv, t, sizeof tv);
    plane_mul_acc(tv, sv, c);
    std::memcpy(t, tv, sizeof tv);
    return RSGPU_OK;
}

// Test hook (not part of include/rsgpu.h): what rsgpu_ec_encode_data_batch
// answers to these arguments with a context at hand, before any device work
// (rsgpu_internal.h ec_batch_args_ok); `tables`: the four tables are given.
int rsgpu_internal_ec_batch_args(int k, int rows, int tables, int max_len, int flags)
{
    return ec_batch_args_ok(k, rows, tables != 0, max_len, flags) ? RSGPU_OK : RSGPU_ERR_ARG;
}

// Test hook (not part of include/rsgpu.h): whether the search's tables of
// rsgpu_correct_blocks' generated form fit the chunk buffers at (k, e, t)
// (rs_jit.hip jit_correct_fits), 1 or 0; -1 for arguments the call refuses.
int rsgpu_internal_jit_correct_fits(int k, int e, int t)
{
    if (k < 1 || e < 1 || e > 64 || k + e > 250 || t < 1 || t > 2)
        return RSGPU_ERR_ARG;
    return jit_correct_fits(k, e, t) ? 1 : 0;
}

// Test hook (not part of include/rsgpu.h): k_rs_bs_correct's pair search
// (rs_pairs.h rs_pair_search_lane) on the host, for the CPU suite to compare
// with the model's brute force: the gf_gen_rs_matrix code (k, e), the syndrome
// column syn [e]; every lane of 64 searches, and the lanes' results combine as
// the kernel's ballots combine them.  Returns the number of matching pairs (0,
// 1, or 2 for several); with 1, out [4] = row a, row b, x_a, x_b.
int rsgpu_internal_rs_pair_search(int k, int e, const unsigned char* syn, int* out)
{
    if (k < 1 || k > 255 || e < 3 || e > 64 || !syn || !out)
        return RSGPU_ERR_ARG;
    static const GfTables gf = make_gf_tables();
    PairGf g;
    for (int i = 0; i < (int)sizeof g; ++i)
        reinterpret_cast<uint8_t*>(&g)[i] = pair_gf_byte(gf, i);
    std::vector<CorRow> row((size_t)k);
    for (int r = 0; r < k; ++r)
        row[r] = rs_pair_row(g, syn[0], syn[1], syn[2], r);
    uint8_t wsyn[64] = {};
    std::memcpy(wsyn, syn, (size_t)e);
    bool several = false;
    int holders = 0;
    CorPairs held{};
    for (int lane = 0; lane < 64; ++lane) {
        const CorPairs c = rs_pair_search_lane(g, k, e, wsyn, row.data(), lane);
        several |= c.cnt >= 2;
        if (c.cnt == 1) {
            ++holders;
            held = c;
        }
    }
    if (several || holders > 1)
        return 2;
    if (holders == 0)
        return 0;
    out[0] = held.ra;
    out[1] = held.rb;
    out[2] = held.xa;
    out[3] = held.xb;
    return 1;
}

// Test hook (not part of include/rsgpu.h): the pair search of k_rs_jit_correct /
// k_rs_jitw_correct (rs_pairs.h pair_search_lane) on the host, the sibling of
// the hook above for any e x k matrix `coef` of a locatable code: the tables
// as the kernel's correct_tables and correct_pending lay them out, every lane
// of 64 searching, the lanes' results combined as the kernel's ballots combine
// them.  Returns 0, 1, or 2 for several; with 1, out [4] = row a, row b, x_a,
// x_b.
int rsgpu_internal_pair_search(int k, int e, const unsigned char* coef, const unsigned char* syn, int* out)
{
    if (k < 1 || k > 255 || e < 3 || e > 64 || !coef || !syn || !out)
        return RSGPU_ERR_ARG;
    static const GfTables gf = make_gf_tables();
    PairGf g;
    for (int i = 0; i < (int)sizeof g; ++i)
        reinterpret_cast<uint8_t*>(&g)[i] = pair_gf_byte(gf, i);
    std::vector<uint8_t> lg(3 * 256);
    for (int r = 0; r < k; ++r)
        for (int p = 0; p < 3; ++p)
            lg[256 * p + r] = pair_log8(gf, coef[(size_t)p * k + r]);
    const unsigned ls0 = pair_logp(&g, syn[0]), ls1 = pair_logp(&g, syn[1]), ls2 = pair_logp(&g, syn[2]);
    std::vector<CorRow> row((size_t)k);
    for (int r = 0; r < k; ++r)
        row[r] = pair_row(&g, ls0, ls1, ls2, lg[r], lg[256 + r], lg[512 + r]);
    bool several = false;
    int holders = 0;
    CorPairs held{};
    for (int lane = 0; lane < 64; ++lane) {
        const CorPairs c = pair_hits(pair_search_lane(
            (const PairGf*)&g, k, e, (const uint8_t*)syn, 1, (const uint8_t*)lg.data(), (const uint8_t*)lg.data() + 256,
            (const uint8_t*)lg.data() + 512, (const CorRow*)row.data(), (const uint8_t*)coef, lane,
            [](unsigned v) { return v; }));
        several |= c.cnt >= 2;
        if (c.cnt == 1) {
            ++holders;
            held = c;
        }
    }
    if (several || holders > 1)
        return 2;
    if (holders == 0)
        return 0;
    out[0] = held.ra;
    out[1] = held.rb;
    out[2] = held.xa;
    out[3] = held.xb;
    return 1;
}

}  // extern "C"
