// rsgpu_scrub.cpp -- the scrub family of the C ABI (include/rsgpu.h): parity
// scrub, repair in place, partial-stripe update, degraded scrub, rebuild in
// place, the locate of several rows and the correction per column.  Argument
// checks and launch sequences; the kernels are rs_kernels.hip (two-pass
// compare, finalise), rs_bitsliced.hip (fused), rs_update.hip, rs_degraded.hip,
// rs_rebuild.hip, rs_locate.hip, rs_correct.hip.  The
// encode and the decode are rsgpu_capi.cpp and rsgpu_decode.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/rsgpu.h"
#include "gf256.h"
#include "rs_kernels.h"
#include "rs_lane.h"
#include "rsgpu_ctx.h"
#include "rsgpu_internal.h"

namespace {

using namespace rsgpu;

// (k, e, matrix): what the device copy of a matrix's tables is kept under
std::vector<uint8_t> matrix_key(int k, int e, const std::vector<uint8_t>& c)
{
    std::vector<uint8_t> key(8 + c.size());
    std::memcpy(key.data(), &k, 4);
    std::memcpy(key.data() + 4, &e, 4);
    std::memcpy(key.data() + 8, c.data(), c.size());
    return key;
}

// rsgpu.h's rule: e >= 2, no zero in rows 0 and 1, the ratios c[1][j] / c[0][j]
// pairwise distinct.  tab (256 bytes, optional): ratio -> j, 255 for none.
bool scrub_locatable(int k, int e, const uint8_t* c, uint8_t* tab)
{
    uint8_t t[256];
    std::memset(t, 255, sizeof t);
    bool ok = e >= 2 && k <= 255;
    for (int j = 0; ok && j < k; ++j) {
        const uint8_t c0 = c[j], c1 = c[(size_t)k + j];
        if (!c0 || !c1) {
            ok = false;
            break;
        }
        const uint8_t ratio = hmul(c1, rsgpu_gf_inv(c0));
        ok = t[ratio] == 255;
        t[ratio] = (uint8_t)j;
    }
    if (ok && tab)
        std::memcpy(tab, t, sizeof t);
    return ok;
}

// the matrix of a call that names rows, and its ratio -> row table
struct Locator {
    std::vector<uint8_t> c;
    uint8_t rowtab[256];
};

// ... or RSGPU_ERR_UNSUPPORTED with `msg` when the matrix is not locatable
int locator(rsgpu_ctx* ctx, int k, int e, const unsigned char* coef, const char* msg, Locator& loc)
{
    if (e >= 2)
        loc.c = parity_matrix(k, e, coef);
    if (e < 2 || !scrub_locatable(k, e, loc.c.data(), loc.rowtab))
        return fail(ctx, RSGPU_ERR_UNSUPPORTED, msg);
    return RSGPU_OK;
}

// the rows the fused kernels of the compiled codes take
bool fused_rows(int k, int e, size_t len, size_t pitch, const void* d_src, const void* d_parity,
                const unsigned char* coef)
{
    return !coef && rs_bitsliced_available(k, e) && len % 32 == 0 && len < (1ull << 32) && pitch % 16 == 0 &&
           (uintptr_t)d_src % 16 == 0 && (uintptr_t)d_parity % 16 == 0;
}

// the fused kernels of the compiled codes (k_rs_bs_scrub, k_rs_bs_repair) serve
bool fused_eligible(const rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, const void* d_src,
                    const void* d_parity, const unsigned char* coef)
{
    return (ctx->scrub_kernel == RSGPU_SCRUB_AUTO || ctx->scrub_kernel == RSGPU_SCRUB_FUSED) &&
           fused_rows(k, e, len, pitch, d_src, d_parity, coef);
}

// Two-pass scratch (ctx->scrub): [rowtab 256 B | matrix e x k | pad to
// kScrubTabBytes | computed parity of a slice].  The parity part is bounded: a
// slice holds as many blocks as fit kScrubParityBytes (4 blocks of C3's 32 x
// 1 MB parity; enough workgroups per launch to fill the device), one block
// when a single block's parity is larger.
constexpr size_t kScrubTabBytes = 16384;  // 256 + e k <= 256 + 125 * 125
constexpr size_t kScrubParityBytes = 128u << 20;

size_t parity_slice(size_t blocks, size_t per_block)
{
    return std::max<size_t>(1, std::min(blocks, kScrubParityBytes / per_block));
}

int grow_parity_scratch(rsgpu_ctx* ctx, size_t blocks, size_t per_block)
{
    return ensure_device(ctx, ctx->scrub, kScrubTabBytes + parity_slice(blocks, per_block) * per_block);
}

// The tables of `loc` at the head of ctx->scrub (>= kScrubTabBytes), uploaded
// when it holds another matrix's
int upload_locator(rsgpu_ctx* ctx, int k, int e, const Locator& loc)
{
    std::vector<uint8_t> key = matrix_key(k, e, loc.c);
    if (key == ctx->scrub.key)
        return RSGPU_OK;
    void* stage;
    int rc = get_stage(ctx, 256 + loc.c.size(), &stage);
    if (rc)
        return rc;
    std::memcpy(stage, loc.rowtab, 256);
    std::memcpy((char*)stage + 256, loc.c.data(), loc.c.size());
    rc = upload(ctx, ctx->scrub.p, 256 + loc.c.size());
    if (!rc)
        ctx->scrub.key = std::move(key);
    return rc;
}

// The rows the generated forms take (k_rs_jit_scrub, k_rs_jit_repair,
// k_rs_jit_locate and their wide kin).  jit_probe probes the device on a
// context's first call: ask only where the call's kernel choice wants the
// generated form, so that no other call ever probes.
bool generated_rows(rsgpu_ctx* ctx, int e, size_t len, size_t pitch, const void* d_src, const void* d_parity)
{
    return rows_aligned(len, pitch, d_src, d_parity) && len < (1ull << 32) && e <= 64 && jit_probe(ctx) == 1;
}

// What a generated slice of nb blocks at src / par needs before its launch:
// the scrub table buffer, the tables of `loc` (when given) at its head, the
// row pointers in the context's scratch, and in s.j the launch of the shared
// program of the matrix c on them.  No parity scratch.
template <class Args>
int generated_prepare(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t nb, const uint8_t* src,
                      const uint8_t* par, const uint8_t* c, const Locator* loc, Args& s)
{
    int rc = ensure_device(ctx, ctx->scrub, kScrubTabBytes);
    if (!rc && loc)
        rc = upload_locator(ctx, k, e, *loc);
    RowPtrs rp;
    if (!rc)
        rc = row_ptr_tables(ctx, k, e, pitch, nb, src, par, rp);
    return rc ? rc : shared_epilogue_args(ctx, c, k, e, (long long)len, rp, s.j);
}

// ... and the launch itself, recorded as `name`
template <class Args>
int generated_launch(rsgpu_ctx* ctx, const Args& s, size_t nb, const char* name,
                     hipError_t (*launch)(const Args&, long long, hipStream_t))
{
    KTimer kt(ctx, name, nb);
    RS_HIP(ctx, launch(s, (long long)nb, ctx->stream));
    return RSGPU_OK;
}

// The two-pass walk over blocks [first, first + count) of d_src: the scratch
// grown, the tables of `loc` (when given) at its head, uploaded when it holds
// another matrix's; then slice by slice the encode into the scratch and
// compare(b0, nb, calc) on blocks [b0, b0 + nb) while their computed parity
// `calc` is still there.
template <class Compare>
int two_pass(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t first, size_t count,
             const uint8_t* d_src, const unsigned char* coef, const Locator* loc, Compare&& compare)
{
    const size_t per_block = (size_t)e * pitch, slice = parity_slice(count, per_block);
    int rc = grow_parity_scratch(ctx, count, per_block);
    if (!rc && loc)
        rc = upload_locator(ctx, k, e, *loc);
    uint8_t* calc = (uint8_t*)ctx->scrub.p + kScrubTabBytes;
    for (size_t b0 = first; !rc && b0 < first + count; b0 += slice) {
        const size_t nb = std::min(slice, first + count - b0);
        rc = rsgpu_encode_blocks(ctx, k, e, len, pitch, nb, d_src + b0 * k * pitch, calc, coef);
        if (!rc)
            rc = compare(b0, nb, calc);
    }
    return rc;
}

// what ScrubCmpArgs and RepairCmpArgs share, for nb blocks of a slice
template <class A, class Fold>
A cmp_args(const rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t nb, const uint8_t* calc,
           decltype(A::par) par, Fold* fold)
{
    A a{};
    a.calc = calc;
    a.par = par;
    a.pitch = (long long)pitch;
    a.len = (long long)len;
    a.blocks = (long long)nb;
    a.k = k;
    a.e = e;
    a.rowtab = (const uint8_t*)ctx->scrub.p;
    a.coef = a.rowtab + 256;
    a.fold = fold;
    return a;
}

// The launches of a kernel that comes as a vector and a byte variant, on nb
// blocks: 16-byte columns [0, n16), then the bytes they leave up to `end` --
// all of them, the tail, or none; with no vector launch the byte launch runs
// even over an empty range (the update then only writes the statuses).
// names: the records of {vector, byte tail, bytes alone}.
template <class Launch>
int launch_head_and_tail(rsgpu_ctx* ctx, const char* const (&names)[3], size_t nb, long long n16, long long end,
                         Launch&& launch)
{
    if (n16 > 0) {
        KTimer kt(ctx, names[0], nb);
        RS_HIP(ctx, launch(false, 0, n16));
    }
    const long long first = n16 * 16;
    if (n16 == 0 || first < end) {
        KTimer kt(ctx, names[n16 > 0 ? 1 : 2], nb);
        RS_HIP(ctx, launch(true, first, std::max(first, end)));
    }
    return RSGPU_OK;
}

constexpr const char* kUpdateNames[3] = {"k_update_blocks", "k_update_blocks(tail)", "k_update_blocks(bytes)"};
constexpr const char* kDegradedNames[3] = {"k_degraded_compare", "k_degraded_compare(tail)",
                                           "k_degraded_compare(bytes)"};
constexpr const char* kRebuildNames[3] = {"k_rebuild_blocks", "k_rebuild_blocks(tail)", "k_rebuild_blocks(bytes)"};
constexpr const char* kLocateNames[3] = {"k_locate_span", "k_locate_span(tail)", "k_locate_span(bytes)"};

// The update's device buffer: [tab4 256 x 16 B | tabc 256 x 4 B | matrix].
constexpr size_t kUpdTab4Bytes = 256 * sizeof(uint4);
constexpr size_t kUpdTabBytes = kUpdTab4Bytes + 256 * sizeof(uint32_t);
constexpr size_t kUpdMatrixBytes = (size_t)RSGPU_MAX_SOURCES * RSGPU_MAX_SOURCES;

// The tables (once per context) and the matrix (when it differs from the one
// the buffer holds) go up on the stream, ahead of the kernel that reads them.
int update_tables(rsgpu_ctx* ctx, int k, int e, const unsigned char* coef)
{
    const bool fresh = ctx->d_update == nullptr;
    if (fresh) {
        RS_HIP(ctx, hipMalloc(&ctx->d_update, kUpdTabBytes + kUpdMatrixBytes));
        ctx->update_key.clear();
    }
    std::vector<uint8_t> c, key;
    if (e > 0) {
        c = parity_matrix(k, e, coef);
        key = matrix_key(k, e, c);
    }
    const bool matrix = e > 0 && key != ctx->update_key;
    if (!fresh && !matrix)
        return RSGPU_OK;
    const size_t first = fresh ? 0 : kUpdTabBytes;
    const size_t last = matrix ? kUpdTabBytes + c.size() : kUpdTabBytes;
    void* stage;
    int rc = get_stage(ctx, kUpdTabBytes + kUpdMatrixBytes, &stage);
    if (rc)
        return rc;
    if (fresh) {
        uint4* t4 = (uint4*)stage;
        uint32_t* tc = (uint32_t*)((char*)stage + kUpdTab4Bytes);
        for (int v = 0; v < 256; ++v) {
            uint32_t t[5];
            perm_tables((uint8_t)v, t);
            t4[v] = make_uint4(t[0], t[1], t[2], t[3]);
            tc[v] = t[4];
        }
    }
    if (matrix)
        std::memcpy((char*)stage + kUpdTabBytes, c.data(), c.size());
    rc = upload(ctx, ctx->d_update, last - first, first, first);
    if (rc)
        return rc;
    if (matrix)
        ctx->update_key = std::move(key);
    return RSGPU_OK;
}

// that buffer as the three fields of UpdateArgs, DegradedArgs or RebuildArgs
template <class Args>
void set_tables(Args& a, const rsgpu_ctx* ctx)
{
    a.tab4 = (const uint4*)ctx->d_update;
    a.tabc = (const uint32_t*)((const char*)ctx->d_update + kUpdTab4Bytes);
    a.coef = (const uint8_t*)ctx->d_update + kUpdTabBytes;
}

bool ranges_overlap(const void* a, size_t an, const void* b, size_t bn)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return an > 0 && bn > 0 && a0 < b0 + bn && b0 < a0 + an;
}

// The per-block tables of one slice (rs_kernels.h DegradedArgs) are bounded as
// the computed parity is: a slice holds no more blocks than fit kDegTabBytes.
constexpr size_t kDegTabBytes = 64u << 20;

constexpr const char* kRebuildPassNames[3] = {"k_rebuild_blocks(pass)", "k_rebuild_blocks(pass)",
                                              "k_rebuild_blocks(pass)"};

size_t round16(size_t n) { return (n + 15) / 16 * 16; }

// What the narrow and the wide rebuild fill alike of RebuildArgs, for blocks
// [g0, g0 + ng); the tables' place and the lane group are the caller's.
RebuildArgs rebuild_args(const rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t g0, size_t ng,
                         unsigned char* d_src, unsigned char* d_parity, int u, const unsigned char* d_lost, bool check,
                         rsgpu_scrub_report* d_report)
{
    const bool work = e > 0 && len > 0;
    RebuildArgs a{};
    a.k = k;
    a.e = e;
    a.u = u;
    a.check = check && work ? 1 : 0;
    a.work = work ? 1 : 0;
    a.pitch = (long long)pitch;
    a.len = (long long)len;
    a.blocks = (long long)ng;
    a.lost = d_lost + g0 * (size_t)u;
    a.src_bytes = rebuild_src_bytes(k);
    a.report = d_report + g0;
    if (work) {
        a.src = d_src + g0 * (size_t)k * pitch;
        a.par = d_parity + g0 * (size_t)e * pitch;
        set_tables(a, ctx);
    }
    return a;
}

// The rebuild of lists that the narrow prepare does not take (u > 8), and of
// any list under THREADED.  Per group of blocks: k_rebuild_wide_prepare, then
//   threaded   k_rs_tc with a row count per block over [0, len - len % 32) and
//              k_rebuild_blocks' byte form, in passes of 8 outputs, over the
//              bytes that leaves
//   otherwise  k_rebuild_blocks in passes of 8 outputs over all of len
// A group's tables (lane tables of the passes; handler addresses, row pointers
// and counts of the threaded code) fit kDegTabBytes, its blocks fit a grid.
int rebuild_wide(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks, unsigned char* d_src,
                 unsigned char* d_parity, const unsigned char* coef, int u, const unsigned char* d_lost, bool check,
                 bool threaded, rsgpu_scrub_report* d_report)
{
    const bool work = e > 0 && len > 0;
    const int most = std::min(u + (check ? 1 : 0), e);  // rows of any block's list as it is rebuilt
    const size_t len32 = threaded ? len - len % 32 : 0;
    const int slots = threaded ? tc_rows_per_pass(most) : 0;
    const int passes = work && len32 < len ? (most + 7) / 8 : 0;
    const size_t lane_stride = (size_t)passes * rebuild_tab_stride(k);
    const size_t per_block = lane_stride + ((size_t)k * slots + k + slots) * 8 + (slots ? 4 : 0);
    const size_t fit = kDegTabBytes / std::max<size_t>(1, per_block);
    size_t group = std::max<size_t>(1, std::min({blocks, kMaxGridBlocks, fit}));
    if (ctx->rebuild_group_max)
        group = std::min(group, ctx->rebuild_group_max);
    rsgpu_ctx::RebuildWideLayout lay;
    lay.blocks = group;
    lay.k = k;
    lay.passes = passes;
    lay.slots = slots;
    lay.lane = 0;
    lay.lane_stride = lane_stride;
    lay.addr = round16(group * lane_stride);
    lay.srcs = lay.addr + group * (size_t)k * slots * 8;
    lay.dsts = lay.srcs + (slots ? group * (size_t)k * 8 : 0);
    lay.count = lay.dsts + group * (size_t)slots * 8;
    int rc = ensure_device(ctx, ctx->rebuild, lay.count + group * 4 + 16);
    if (rc)
        return rc;
    ctx->rebuild_wide = lay;
    if (work) {
        // the v_perm tables of every coefficient value and the matrix, on the device
        rc = update_tables(ctx, k, e, coef);
        if (rc)
            return rc;
    }
    char* base = (char*)ctx->rebuild.p;
    for (size_t g0 = 0; g0 < blocks; g0 += group) {
        const size_t ng = std::min(group, blocks - g0);
        RebuildWideArgs wa{};
        RebuildArgs& a = wa.r;
        a = rebuild_args(ctx, k, e, len, pitch, g0, ng, d_src, d_parity, u, d_lost, check, d_report);
        a.tab = passes ? (uint8_t*)base + lay.lane : nullptr;
        a.tab_stride = lane_stride;
        wa.passes = passes;
        wa.slots = slots;
        if (slots) {
            wa.tc_table = ctx->d_tc_table;
            wa.addr = (unsigned long long*)(base + lay.addr);
            wa.srcs = (const uint8_t**)(base + lay.srcs);
            wa.dsts = (uint8_t**)(base + lay.dsts);
            wa.count = (int*)(base + lay.count);
        }
        {
            KTimer kt(ctx, "k_rebuild_wide_prepare", ng);
            RS_HIP(ctx, launch_rebuild_wide_prepare(wa, ctx->stream));
        }
        if (!work || ctx->rebuild_prepare_only)
            continue;  // the prepare has written every report
        if (slots) {
            const TcArgs t = tc_args(wa.srcs, wa.dsts, slots, wa.addr, (long long)k * slots, k, most,
                                     (long long)len32, wa.count);
            KTimer kt(ctx, "k_rs_tc(rebuild)", ng);
            RS_HIP(ctx, launch_rs_tc_counted(t, (long long)ng, ctx->stream));
        }
        // the lane kernel on what is left, a pass of at most 8 outputs at a time
        const bool vec = !slots && ptrs_aligned(pitch, d_src, d_parity);
        const long long n16 = vec ? (long long)(len / 16) : 0;
        for (int p = 0; p < passes; ++p) {
            RebuildArgs pa = a;
            pa.u = std::min(8, most - 8 * p);  // this pass's most rows: the launcher's G
            pa.check = 0;
            pa.tab = a.tab + (size_t)p * rebuild_tab_stride(k);
            pa.g = lane_group(pa.u);
            auto launch = [&](bool bytes, long long c0, long long c1) {
                return launch_rebuild_blocks(pa, bytes, c0, c1, ctx->stream);
            };
            if (slots) {
                KTimer kt(ctx, kRebuildPassNames[0], ng);
                RS_HIP(ctx, launch(true, (long long)len32, (long long)len));
            } else {
                rc = launch_head_and_tail(ctx, kRebuildPassNames, ng, n16, (long long)len, launch);
                if (rc)
                    return rc;
            }
        }
    }
    return RSGPU_OK;
}

// the six kernel choices: 0 (AUTO) to `last` into the context's member
int set_kernel(rsgpu_ctx* ctx, int kernel, int last, int rsgpu_ctx::*choice, const char* msg)
{
    if (!ctx || kernel < 0 || kernel > last)
        return fail(ctx, RSGPU_ERR_ARG, msg);
    ctx->*choice = kernel;
    return RSGPU_OK;
}

}  // namespace

extern "C" {

int rsgpu_scrub_locatable(int k, int e, const unsigned char* coef)
{
    if (k <= 0 || e < 2 || k + e > RSGPU_MAX_SOURCES)
        return 0;
    const std::vector<uint8_t> c = parity_matrix(k, e, coef);
    return scrub_locatable(k, e, c.data(), nullptr) ? 1 : 0;
}

int rsgpu_set_scrub_kernel(rsgpu_ctx* ctx, int kernel)
{
    return set_kernel(ctx, kernel, RSGPU_SCRUB_GENERATED, &rsgpu_ctx::scrub_kernel, "rsgpu_set_scrub_kernel: unknown kernel");
}

int rsgpu_set_rebuild_kernel(rsgpu_ctx* ctx, int kernel)
{
    return set_kernel(ctx, kernel, RSGPU_REBUILD_THREADED, &rsgpu_ctx::rebuild_kernel, "rsgpu_set_rebuild_kernel: unknown kernel");
}

int rsgpu_set_locate_kernel(rsgpu_ctx* ctx, int kernel)
{
    return set_kernel(ctx, kernel, RSGPU_LOCATE_FUSED, &rsgpu_ctx::locate_kernel, "rsgpu_set_locate_kernel: unknown kernel");
}

int rsgpu_set_degraded_kernel(rsgpu_ctx* ctx, int kernel)
{
    return set_kernel(ctx, kernel, RSGPU_DEGRADED_FUSED, &rsgpu_ctx::degraded_kernel, "rsgpu_set_degraded_kernel: unknown kernel");
}

int rsgpu_set_correct_kernel(rsgpu_ctx* ctx, int kernel)
{
    return set_kernel(ctx, kernel, RSGPU_CORRECT_FUSED, &rsgpu_ctx::correct_kernel, "rsgpu_set_correct_kernel: unknown kernel");
}

int rsgpu_set_repair_kernel(rsgpu_ctx* ctx, int kernel)
{
    return set_kernel(ctx, kernel, RSGPU_REPAIR_KERNEL_GENERATED, &rsgpu_ctx::repair_kernel, "rsgpu_set_repair_kernel: unknown kernel");
}

int rsgpu_scrub_blocks(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                       const unsigned char* d_src, const unsigned char* d_parity,
                       const unsigned char* coef, int flags, rsgpu_scrub_report* d_report)
{
    int rc = check_geom(ctx, k, e, len, pitch, blocks);
    if (rc)
        return rc;
    if (!d_report || (uintptr_t)d_report % 8 != 0 || (flags & ~RSGPU_SCRUB_LOCATE) != 0)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_scrub_blocks: bad report pointer or flags");
    const bool locate = (flags & RSGPU_SCRUB_LOCATE) != 0;
    const bool work = e > 0 && len > 0;
    if (work && (!d_src || !d_parity))
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_scrub_blocks: null rows");
    Locator loc;
    if (locate) {
        rc = locator(ctx, k, e, coef,
                     "rsgpu_scrub_blocks: RSGPU_SCRUB_LOCATE needs a locatable matrix (rsgpu_scrub_locatable)", loc);
        if (rc)
            return rc;
    }
    ScrubFold* fold = reinterpret_cast<ScrubFold*>(d_report);
    RS_HIP(ctx, hipMemsetAsync(d_report, 0, blocks * sizeof(rsgpu_scrub_report), ctx->stream));
    auto compare = [&](size_t b0, size_t nb, const uint8_t* calc) -> int {
        ScrubCmpArgs a =
            cmp_args<ScrubCmpArgs>(ctx, k, e, len, pitch, nb, calc, d_parity + b0 * e * pitch, fold + b0);
        a.locate = locate ? 1 : 0;
        KTimer kt(ctx, "k_scrub_compare", nb);
        RS_HIP(ctx, launch_scrub_compare(a, ctx->stream));
        return RSGPU_OK;
    };
    const bool fused = fused_eligible(ctx, k, e, len, pitch, d_src, d_parity, coef);
    // GENERATED: any matrix, with or without `coef` (rsgpu.h)
    const bool generated = work && ctx->scrub_kernel == RSGPU_SCRUB_GENERATED &&
                           generated_rows(ctx, e, len, pitch, d_src, d_parity);
    // the matrix's shared program on a slice, the stored parity compared in
    // registers; the locate tables where the two-pass scratch has them
    auto generated_slice = [&](size_t b0, size_t nb) -> int {
        const std::vector<uint8_t> c = locate ? loc.c : parity_matrix(k, e, coef);
        JitScrubArgs s{};
        const int grc = generated_prepare(ctx, k, e, len, pitch, nb, d_src + b0 * k * pitch, d_parity + b0 * e * pitch,
                                          c.data(), locate ? &loc : nullptr, s);
        s.fold = fold + b0;
        s.tab = (const uint8_t*)ctx->scrub.p;
        s.locate = locate ? 1 : 0;
        return grc ? grc : generated_launch(ctx, s, nb, "k_rs_jit_scrub", launch_rs_jit_scrub);
    };
    rc = for_grid_slices(work ? blocks : 0, [&](size_t b0, size_t nb) -> int {
        if (generated)
            return generated_slice(b0, nb);
        if (!fused)
            return two_pass(ctx, k, e, len, pitch, b0, nb, d_src, coef, locate ? &loc : nullptr, compare);
        KTimer kt(ctx, "k_rs_bs_scrub", nb);
        RS_HIP(ctx, launch_rs_bitsliced_scrub(k, e, d_src + b0 * k * pitch, d_parity + b0 * e * pitch,
                                              (long long)pitch, (long long)len, (long long)nb, fold + b0,
                                              locate ? 1 : 0, ctx->stream));
        return RSGPU_OK;
    });
    if (rc)
        return rc;
    KTimer kt(ctx, "k_scrub_finalise", blocks);
    RS_HIP(ctx, launch_scrub_finalise(d_report, (long long)blocks, locate ? 1 : 0, ctx->stream));
    return RSGPU_OK;
}

int rsgpu_repair_blocks(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                        unsigned char* d_src, unsigned char* d_parity, const unsigned char* coef, int mode,
                        rsgpu_repair_report* d_report)
{
    int rc = check_geom(ctx, k, e, len, pitch, blocks);
    if (rc)
        return rc;
    if (!d_report || (uintptr_t)d_report % 8 != 0 ||
        (mode != RSGPU_REPAIR_ONE_ROW && mode != RSGPU_REPAIR_COLUMNS))
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_repair_blocks: bad report pointer or mode");
    const bool work = e > 0 && len > 0;
    if (work && (!d_src || !d_parity))
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_repair_blocks: null rows");
    Locator loc;
    if (e > 0) {  // e == 0: no parity, nothing can be bad
        rc = locator(ctx, k, e, coef, "rsgpu_repair_blocks: needs a locatable matrix (rsgpu_scrub_locatable)", loc);
        if (rc)
            return rc;
        if (mode == RSGPU_REPAIR_COLUMNS && e < 3)
            return fail(ctx, RSGPU_ERR_UNSUPPORTED, "rsgpu_repair_blocks: RSGPU_REPAIR_COLUMNS needs e >= 3");
    }
    RepairFold* fold = reinterpret_cast<RepairFold*>(d_report);
    RS_HIP(ctx, hipMemsetAsync(d_report, 0, blocks * sizeof(rsgpu_repair_report), ctx->stream));
    auto finalise = [&](size_t b0, size_t nb) -> int {
        KTimer kt(ctx, "k_repair_finalise", nb);
        RS_HIP(ctx, launch_repair_finalise(fold + b0, (long long)nb, mode, ctx->stream));
        return RSGPU_OK;
    };
    if (!work)
        return finalise(0, blocks);
    // GENERATED (rsgpu_set_repair_kernel): any matrix, with or without `coef`,
    // on the rows the generated scrub takes; before FUSED where both apply
    const bool generated = ctx->repair_kernel == RSGPU_REPAIR_KERNEL_GENERATED &&
                           generated_rows(ctx, e, len, pitch, d_src, d_parity);
    const bool fused = !generated && fused_eligible(ctx, k, e, len, pitch, d_src, d_parity, coef);
    const int first_mode = mode == RSGPU_REPAIR_COLUMNS ? kRepairColumns : kRepairLocate;
    // The matrix's shared program on a slice, correcting in its cold path, as
    // the generated scrub.  ONE_ROW: the launch that only folds, the finalise
    // of the slice's reports, and the gated correcting launch on the same row
    // pointers.
    auto generated_slice = [&](size_t b0, size_t nb) -> int {
        JitRepairArgs s{};
        s.src = d_src + b0 * k * pitch;
        s.par = d_parity + b0 * e * pitch;
        int grc = generated_prepare(ctx, k, e, len, pitch, nb, s.src, s.par, loc.c.data(), &loc, s);
        s.fold = fold + b0;
        s.tab = (const uint8_t*)ctx->scrub.p;
        s.pitch = (long long)pitch;
        s.mode = first_mode;
        if (!grc)
            grc = generated_launch(ctx, s, nb, "k_rs_jit_repair", launch_rs_jit_repair);
        if (!grc)
            grc = finalise(b0, nb);
        s.mode = kRepairGated;
        if (!grc && mode == RSGPU_REPAIR_ONE_ROW)
            grc = generated_launch(ctx, s, nb, "k_rs_jit_repair_gated", launch_rs_jit_repair);
        return grc;
    };
    // A slice of the scratch.  COLUMNS: the correcting compare; ONE_ROW: the
    // compare that only folds, the finalise of the slice's reports, and the
    // gated correcting compare, while the slice's computed parity is still in
    // the scratch.
    auto compare = [&](size_t b0, size_t nb, const uint8_t* calc) -> int {
        RepairCmpArgs a =
            cmp_args<RepairCmpArgs>(ctx, k, e, len, pitch, nb, calc, d_parity + b0 * e * pitch, fold + b0);
        a.src = d_src + b0 * k * pitch;
        a.mode = first_mode;
        {
            KTimer kt(ctx, "k_repair_compare", nb);
            RS_HIP(ctx, launch_repair_compare(a, ctx->stream));
        }
        if (mode != RSGPU_REPAIR_ONE_ROW)
            return RSGPU_OK;
        const int frc = finalise(b0, nb);
        if (frc)
            return frc;
        a.mode = kRepairGated;
        KTimer kt(ctx, "k_repair_compare_gated", nb);
        RS_HIP(ctx, launch_repair_compare(a, ctx->stream));
        return RSGPU_OK;
    };
    // block index in grid.y: larger batches as consecutive slices, each
    // complete (located, finalised, corrected) before the next
    return for_grid_slices(blocks, [&](size_t b0, size_t nb) -> int {
        uint8_t* src = d_src + b0 * k * pitch;
        uint8_t* par = d_parity + b0 * e * pitch;
        if (generated)
            return generated_slice(b0, nb);
        if (!fused) {
            rc = two_pass(ctx, k, e, len, pitch, b0, nb, d_src, coef, &loc, compare);
            if (rc || mode == RSGPU_REPAIR_ONE_ROW)
                return rc;  // ONE_ROW: finalised slice by slice
        } else {
            KTimer kt(ctx, "k_rs_bs_repair", nb);
            RS_HIP(ctx, launch_rs_bitsliced_repair(k, e, src, par, (long long)pitch, (long long)len, (long long)nb,
                                                   fold + b0, first_mode, ctx->stream));
        }
        rc = finalise(b0, nb);
        if (rc)
            return rc;
        if (fused && mode == RSGPU_REPAIR_ONE_ROW) {
            KTimer kt(ctx, "k_rs_bs_repair_gated", nb);
            RS_HIP(ctx, launch_rs_bitsliced_repair(k, e, src, par, (long long)pitch, (long long)len, (long long)nb,
                                                   fold + b0, kRepairGated, ctx->stream));
        }
        return RSGPU_OK;
    });
}

int rsgpu_correct_blocks(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                         unsigned char* d_src, unsigned char* d_parity, const unsigned char* coef, int t,
                         rsgpu_correct_report* d_report)
{
    int rc = check_geom(ctx, k, e, len, pitch, blocks);
    if (rc)
        return rc;
    if (!d_report || (uintptr_t)d_report % 8 != 0 || (t != 1 && t != 2))
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_correct_blocks: bad report pointer or t");
    const bool work = e > 0 && len > 0;
    if (work && (!d_src || !d_parity))
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_correct_blocks: null rows");
    Locator loc;
    if (e > 0) {  // e == 0: no parity, nothing can be bad
        rc = locator(ctx, k, e, coef, "rsgpu_correct_blocks: needs a locatable matrix (rsgpu_scrub_locatable)", loc);
        if (rc)
            return rc;
        if (t == 1 && e < 3)
            return fail(ctx, RSGPU_ERR_UNSUPPORTED, "rsgpu_correct_blocks: t == 1 needs e >= 3");
        if (t == 2 && (e < 5 || e > 64))
            return fail(ctx, RSGPU_ERR_UNSUPPORTED, "rsgpu_correct_blocks: t == 2 needs 5 <= e <= 64");
    }
    CorrectFold* fold = reinterpret_cast<CorrectFold*>(d_report);
    RS_HIP(ctx, hipMemsetAsync(d_report, 0, blocks * sizeof(rsgpu_correct_report), ctx->stream));
    // TWO_PASS (and AUTO): per slice of the scratch the encode, then the
    // correcting compare while the slice's computed parity is still there
    auto compare = [&](size_t b0, size_t nb, const uint8_t* calc) -> int {
        CorrectCmpArgs a =
            cmp_args<CorrectCmpArgs>(ctx, k, e, len, pitch, nb, calc, d_parity + b0 * e * pitch, fold + b0);
        a.src = d_src + b0 * k * pitch;
        a.t = t;
        KTimer kt(ctx, "k_correct_compare", nb);
        RS_HIP(ctx, launch_correct_compare(a, ctx->stream));
        return RSGPU_OK;
    };
    // FUSED (rsgpu_set_correct_kernel), on the rows the fused kernels take: a
    // slice is one launch of the compiled code's kernel, which compares in
    // registers and corrects in its cold path; no scratch, no locate tables
    const bool want_fused = work && ctx->correct_kernel == RSGPU_CORRECT_FUSED;
    const bool fused = want_fused && fused_rows(k, e, len, pitch, d_src, d_parity, coef);
    // Where the compiled form does not apply and the context's scrub kernel is
    // GENERATED, the generated form: a slice is one k_rs_jit_correct /
    // k_rs_jitw_correct on the matrix's shared program, row pointers in the
    // context's scratch as the GENERATED scrub builds them; no encode, and the
    // parity scratch neither touched nor grown
    const bool generated = want_fused && !fused && ctx->scrub_kernel == RSGPU_SCRUB_GENERATED &&
                           jit_correct_fits(k, e, t) && generated_rows(ctx, e, len, pitch, d_src, d_parity);
    // block index in grid.y: larger batches as consecutive slices
    rc = for_grid_slices(work ? blocks : 0, [&](size_t b0, size_t nb) -> int {
        if (generated) {
            JitCorrectArgs s{};
            s.src = d_src + b0 * k * pitch;
            s.par = d_parity + b0 * e * pitch;
            const int grc = generated_prepare(ctx, k, e, len, pitch, nb, s.src, s.par, loc.c.data(), &loc, s);
            s.fold = fold + b0;
            s.tab = (const uint8_t*)ctx->scrub.p;
            s.pitch = (long long)pitch;
            s.t = t;
            return grc ? grc : generated_launch(ctx, s, nb, "k_rs_jit_correct", launch_rs_jit_correct);
        }
        if (!fused)
            return two_pass(ctx, k, e, len, pitch, b0, nb, d_src, coef, &loc, compare);
        KTimer kt(ctx, "k_rs_bs_correct", nb);
        RS_HIP(ctx, launch_rs_bitsliced_correct(k, e, d_src + b0 * k * pitch, d_parity + b0 * e * pitch,
                                                (long long)pitch, (long long)len, (long long)nb, fold + b0, t,
                                                ctx->stream));
        return RSGPU_OK;
    });
    if (rc)
        return rc;
    KTimer kt(ctx, "k_correct_finalise", blocks);
    RS_HIP(ctx, launch_correct_finalise(d_report, (long long)blocks, ctx->stream));
    return RSGPU_OK;
}

int rsgpu_update_blocks(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks, int u,
                        const unsigned char* d_cols, const unsigned char* d_upd, unsigned char* d_src,
                        unsigned char* d_parity, const unsigned char* coef, int flags, int* d_status)
{
    int rc = check_geom(ctx, k, e, len, pitch, blocks);
    if (rc)
        return rc;
    if (u < 1 || u > k || (flags & ~RSGPU_UPDATE_DELTA) != 0 || !d_cols || !d_status)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_update_blocks: bad u, flags, list or status pointer");
    const bool delta = (flags & RSGPU_UPDATE_DELTA) != 0;
    const bool src_used = !delta, par_used = e > 0;
    if (len > 0 && (((src_used || par_used) && !d_upd) || (src_used && !d_src) || (par_used && !d_parity)))
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_update_blocks: null rows");
    // rows i of a buffer of R rows per block end at ((blocks R - 1) pitch + len)
    auto span = [&](size_t rows) { return len == 0 ? (size_t)0 : (blocks * rows - 1) * pitch + len; };
    if ((src_used && ranges_overlap(d_upd, span((size_t)u), d_src, span((size_t)k))) ||
        (par_used && ranges_overlap(d_upd, span((size_t)u), d_parity, span((size_t)e))))
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_update_blocks: d_upd overlaps d_src or d_parity");
    rc = update_tables(ctx, k, e, coef);
    if (rc)
        return rc;
    const bool work = len > 0 && (src_used || par_used);
    const bool vec = pitch % 16 == 0 && (uintptr_t)d_upd % 16 == 0 && (!src_used || (uintptr_t)d_src % 16 == 0) &&
                     (!par_used || (uintptr_t)d_parity % 16 == 0);
    const long long n16 = work && vec ? (long long)(len / 16) : 0;
    return for_grid_slices(blocks, [&](size_t b0, size_t nb) {
        UpdateArgs a{};
        a.k = k;
        a.e = e;
        a.u = u;
        a.delta = delta ? 1 : 0;
        a.pitch = (long long)pitch;
        a.blocks = (long long)nb;
        a.cols = d_cols + b0 * (size_t)u;
        a.upd = d_upd ? d_upd + b0 * (size_t)u * pitch : nullptr;
        a.src = src_used && d_src ? d_src + b0 * (size_t)k * pitch : nullptr;
        a.par = par_used && d_parity ? d_parity + b0 * (size_t)e * pitch : nullptr;
        set_tables(a, ctx);
        a.status = d_status + b0;
        auto launch = [&](bool bytes, long long c0, long long c1) {
            return launch_update_blocks(a, bytes, c0, c1, ctx->stream);
        };
        return launch_head_and_tail(ctx, kUpdateNames, nb, n16, work ? (long long)len : 0, launch);
    });
}

int rsgpu_scrub_degraded_blocks(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                                const unsigned char* d_src, const unsigned char* d_parity,
                                const unsigned char* coef, int u, const unsigned char* d_lost, int flags,
                                rsgpu_scrub_report* d_report)
{
    int rc = check_geom(ctx, k, e, len, pitch, blocks);
    if (rc)
        return rc;
    if (!d_report || (uintptr_t)d_report % 8 != 0 || (flags & ~RSGPU_SCRUB_LOCATE) != 0 || u < 1 || u > 8 ||
        !d_lost)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_scrub_degraded_blocks: bad report pointer, flags, u or list");
    const bool work = e > 0 && len > 0;
    if (work && (!d_src || !d_parity))
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_scrub_degraded_blocks: null rows");
    // Two nested slicings.  A group of blocks shares one prepare and one
    // finalise: its tables fit kDegTabBytes, its blocks fit a grid.  Inside it
    // a slice is what the scrub scratch holds of computed parity (the TWO_PASS
    // rule): encode, then compare.  FUSED (rsgpu_set_degraded_kernel) on the
    // rows the fused scrub takes: one k_rs_bs_degraded launch over the group
    // in their place, no encode and no parity scratch.  Where the compiled
    // form does not apply and the context's scrub kernel is GENERATED, the
    // generated form: per group one k_rs_jit_degraded / k_rs_jitw_degraded on
    // the matrix's shared program, row pointers in the context's scratch as
    // the GENERATED scrub builds them, for any matrix; no encode, and the
    // parity scratch neither touched nor grown.
    const size_t per_block = (size_t)e * pitch, stride = degraded_tab_stride(k, e);
    size_t group = std::max<size_t>(1, std::min({blocks, kMaxGridBlocks, kDegTabBytes / stride}));
    if (ctx->degraded_group_max)
        group = std::min(group, ctx->degraded_group_max);
    rc = ensure_device(ctx, ctx->degraded, group * stride);
    if (rc)
        return rc;
    const bool want_fused = work && ctx->degraded_kernel == RSGPU_DEGRADED_FUSED;
    const bool compiled = want_fused && fused_rows(k, e, len, pitch, d_src, d_parity, coef);
    const bool generated = want_fused && !compiled && ctx->scrub_kernel == RSGPU_SCRUB_GENERATED &&
                           generated_rows(ctx, e, len, pitch, d_src, d_parity);
    const bool fused = compiled || generated;
    const std::vector<uint8_t> matrix = generated ? parity_matrix(k, e, coef) : std::vector<uint8_t>();
    if (work) {
        // the scratch of the largest group now, so that no walk below grows it
        rc = fused ? RSGPU_OK : grow_parity_scratch(ctx, group, per_block);
        // generated: the row pointers of the largest group, [group][k] then
        // [group][e], before any group's prepare is enqueued (a growth waits
        // for the stream and frees the old buffer).  H comes from the block's
        // table, so the scrub's table buffer (ctx->scrub) is not needed.
        if (!rc && generated)
            rc = ensure_scratch(ctx, align_up(sizeof(void*) * (size_t)k * group, 256) +
                                         align_up(sizeof(void*) * (size_t)e * group, 256));
        if (rc)
            return rc;
        // the v_perm tables of every coefficient value and the matrix, on the device
        rc = update_tables(ctx, k, e, coef);
        if (rc)
            return rc;
    }
    const bool vec = pitch % 16 == 0 && (uintptr_t)d_parity % 16 == 0;
    const long long n16 = work && vec ? (long long)(len / 16) : 0;
    for (size_t g0 = 0; g0 < blocks; g0 += group) {
        const size_t ng = std::min(group, blocks - g0);
        DegradedArgs a{};
        a.k = k;
        a.e = e;
        a.u = u;
        a.locate = (flags & RSGPU_SCRUB_LOCATE) ? 1 : 0;
        a.work = work ? 1 : 0;
        a.pitch = (long long)pitch;
        a.len = (long long)len;
        a.blocks = (long long)ng;
        a.lost = d_lost + g0 * (size_t)u;
        a.tab = (uint8_t*)ctx->degraded.p;
        a.tab_stride = stride;
        a.rest_bytes = degraded_rest_bytes(e);
        a.report = d_report + g0;
        if (work)
            set_tables(a, ctx);
        // generated: the group's row pointers and the matrix's program (built
        // on first use) before the prepare is enqueued; the launch follows it
        JitDegradedArgs js{};
        if (generated) {
            RowPtrs rp;
            rc = row_ptr_tables(ctx, k, e, pitch, ng, d_src + g0 * (size_t)k * pitch, d_parity + g0 * per_block, rp);
            if (!rc)
                rc = shared_epilogue_args(ctx, matrix.data(), k, e, (long long)len, rp, js.j);
            if (rc)
                return rc;
            js.tab = a.tab;
            js.tab_stride = stride;
            js.fold = reinterpret_cast<ScrubFold*>(d_report + g0);
            js.locate = a.locate;
        }
        {
            KTimer kt(ctx, "k_degraded_prepare", ng);
            RS_HIP(ctx, launch_degraded_prepare(a, ctx->stream));
        }
        if (!work)
            continue;  // the prepare has written every report
        // the parity of the k source rows as they lie in memory, lost ones
        // included: their contribution cancels in the reduced syndromes
        auto compare = [&](size_t b0, size_t nb, const uint8_t* calc) {
            DegradedArgs c = a;
            c.blocks = (long long)nb;
            c.tab = a.tab + (b0 - g0) * stride;
            c.report = d_report + b0;
            c.calc = calc;
            c.par = d_parity + b0 * per_block;
            auto launch = [&](bool bytes, long long c0, long long c1) {
                return launch_degraded_compare(c, bytes, c0, c1, ctx->stream);
            };
            return launch_head_and_tail(ctx, kDegradedNames, nb, n16, (long long)len, launch);
        };
        if (generated) {
            rc = generated_launch(ctx, js, ng, "k_rs_jit_degraded", launch_rs_jit_degraded);
            if (rc)
                return rc;
        } else if (compiled) {
            KTimer kt(ctx, "k_rs_bs_degraded", ng);
            RS_HIP(ctx, launch_rs_bitsliced_degraded(k, e, d_src + g0 * (size_t)k * pitch, d_parity + g0 * per_block,
                                                     (long long)pitch, (long long)len, (long long)ng, a.tab,
                                                     reinterpret_cast<ScrubFold*>(d_report + g0), a.locate,
                                                     ctx->stream));
        } else {
            rc = two_pass(ctx, k, e, len, pitch, g0, ng, d_src, coef, nullptr, compare);
            if (rc)
                return rc;
        }
        KTimer kt(ctx, "k_degraded_finalise", ng);
        RS_HIP(ctx, launch_degraded_finalise(a, ctx->stream));
    }
    return RSGPU_OK;
}

int rsgpu_rebuild_blocks(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                         unsigned char* d_src, unsigned char* d_parity, const unsigned char* coef, int u,
                         const unsigned char* d_lost, int flags, rsgpu_scrub_report* d_report)
{
    int rc = check_geom(ctx, k, e, len, pitch, blocks);
    if (rc)
        return rc;
    const bool check = (flags & RSGPU_REBUILD_CHECK) != 0;
    // with the check the located row may join the list, and the compare's lanes
    // hold 8 rows; without it a list is as long as the code has parity rows
    const int umax = check ? 7 : std::max(8, std::min(e, RSGPU_REBUILD_MAX_LOST));
    if (!d_report || (uintptr_t)d_report % 8 != 0 || (flags & ~RSGPU_REBUILD_CHECK) != 0 || u < 1 || u > umax ||
        !d_lost)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_rebuild_blocks: bad report pointer, flags, u or list");
    const bool work = e > 0 && len > 0;
    if (work && (!d_src || !d_parity))
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_rebuild_blocks: null rows");
    // the verdict on every block as it is now; the prepare below acts on it.
    // With nothing to check the prepare alone judges the lists.
    if (check && work) {
        rc = rsgpu_scrub_degraded_blocks(ctx, k, e, len, pitch, blocks, d_src, d_parity, coef, u, d_lost,
                                         RSGPU_SCRUB_LOCATE, d_report);
        if (rc)
            return rc;
    }
    const bool vec = ptrs_aligned(pitch, d_src, d_parity);
    // the kernel: AUTO changes nothing for u + check <= 8
    const bool long_list = u + (check ? 1 : 0) > 8;
    const bool threaded = work && vec && len >= 32 && len < (1ull << 32) &&
                          (ctx->rebuild_kernel == RSGPU_REBUILD_THREADED ||
                           (ctx->rebuild_kernel == RSGPU_REBUILD_AUTO && long_list)) &&
                          tc_handlers_ready(ctx);
    if (threaded || long_list)
        return rebuild_wide(ctx, k, e, len, pitch, blocks, d_src, d_parity, coef, u, d_lost, check, threaded,
                            d_report);
    // a group of blocks shares one prepare: its tables fit kDegTabBytes, its
    // blocks fit a grid
    const size_t stride = rebuild_tab_stride(k);
    const size_t group = std::max<size_t>(1, std::min({blocks, kMaxGridBlocks, kDegTabBytes / stride}));
    rc = ensure_device(ctx, ctx->rebuild, group * stride);
    if (rc)
        return rc;
    if (work) {
        // the v_perm tables of every coefficient value and the matrix, on the device
        rc = update_tables(ctx, k, e, coef);
        if (rc)
            return rc;
    }
    const long long n16 = work && vec ? (long long)(len / 16) : 0;
    const int most = std::min(u + (check ? 1 : 0), e);  // rows of any block's list as it is rebuilt
    for (size_t g0 = 0; g0 < blocks; g0 += group) {
        const size_t ng = std::min(group, blocks - g0);
        RebuildArgs a = rebuild_args(ctx, k, e, len, pitch, g0, ng, d_src, d_parity, u, d_lost, check, d_report);
        a.tab = (uint8_t*)ctx->rebuild.p;
        a.tab_stride = stride;
        a.g = lane_group(most);
        {
            KTimer kt(ctx, "k_rebuild_prepare", ng);
            RS_HIP(ctx, launch_rebuild_prepare(a, ctx->stream));
        }
        if (!work)
            continue;  // the prepare has written every report
        auto launch = [&](bool bytes, long long c0, long long c1) {
            return launch_rebuild_blocks(a, bytes, c0, c1, ctx->stream);
        };
        rc = launch_head_and_tail(ctx, kRebuildNames, ng, n16, (long long)len, launch);
        if (rc)
            return rc;
    }
    return RSGPU_OK;
}

int rsgpu_locate_blocks(rsgpu_ctx* ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                        const unsigned char* d_src, const unsigned char* d_parity, const unsigned char* coef, int u,
                        unsigned char* d_rows, rsgpu_scrub_report* d_report)
{
    int rc = check_geom(ctx, k, e, len, pitch, blocks);
    if (rc)
        return rc;
    if (!d_report || (uintptr_t)d_report % 8 != 0 || u < 1 || u > RSGPU_LOCATE_MAX_ROWS || !d_rows)
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_locate_blocks: bad report pointer, u or list");
    const bool work = e > 0 && len > 0;
    if (work && (!d_src || !d_parity))
        return fail(ctx, RSGPU_ERR_ARG, "rsgpu_locate_blocks: null rows");
    if (e > 64)  // a lane of the wave per syndrome
        return fail(ctx, RSGPU_ERR_UNSUPPORTED, "rsgpu_locate_blocks: needs e <= 64");
    // Two nested slicings, as the degraded scrub's.  A group of blocks shares
    // one finish: its candidate areas fit kDegTabBytes, its blocks fit a grid.
    // Inside it a slice is what the scrub scratch holds of computed parity
    // (the TWO_PASS rule): encode, then span.  A block's area has one slot
    // per workgroup of the vector launch, then one per workgroup of the byte
    // launch; the workgroups per block are those of the largest slice.
    // FUSED (rsgpu.h): per group one k_rs_bs_locate, which reads the rows as
    // the FUSED scrub does and leaves a slot per dirty tile, the block's area
    // holding one per tile; no scratch, no encode.  Where the compiled form
    // does not apply and the context's scrub kernel is GENERATED, the
    // generated form: per group one k_rs_jit_locate / k_rs_jitw_locate on the
    // matrix's shared program, row pointers in the context's scratch as the
    // GENERATED scrub builds them, the same slots and the same finish.
    const size_t per_block = (size_t)e * pitch;
    const size_t tiles = (len + 2047) / 2048;
    const bool want_fused = work && ctx->locate_kernel == RSGPU_LOCATE_FUSED &&
                            tiles * kLocateSlotBytes <= kDegTabBytes;
    const bool compiled = want_fused && fused_rows(k, e, len, pitch, d_src, d_parity, coef);
    const bool generated = want_fused && !compiled && ctx->scrub_kernel == RSGPU_SCRUB_GENERATED &&
                           generated_rows(ctx, e, len, pitch, d_src, d_parity);
    const bool fused = compiled || generated;
    const bool vec = pitch % 16 == 0 && (uintptr_t)d_parity % 16 == 0;
    const long long n16 = work && vec ? (long long)(len / 16) : 0;
    const long long rest = (long long)len - n16 * 16;  // byte columns
    unsigned gx_vec = 0, gx_bytes = 0;
    if (work && !fused) {
        const long long most = (long long)parity_slice(std::min(blocks, kMaxGridBlocks), per_block);
        gx_vec = n16 > 0 ? columns_grid_x(n16, most, 256) : 0;
        gx_bytes = rest > 0 ? columns_grid_x(rest, most, 256) : 0;
    }
    const int slots = fused ? (int)tiles : (int)(gx_vec + gx_bytes);
    const size_t stride = (size_t)slots * kLocateSlotBytes;
    size_t group = std::max<size_t>(1, std::min({blocks, kMaxGridBlocks, kDegTabBytes / std::max<size_t>(1, stride)}));
    if (ctx->locate_group_max)
        group = std::min(group, ctx->locate_group_max);
    const std::vector<uint8_t> matrix = generated ? parity_matrix(k, e, coef) : std::vector<uint8_t>();
    if (work) {
        rc = ensure_device(ctx, ctx->locate, group * stride);
        // the scratch of the largest group now, so that no walk below grows it
        if (!rc && !fused)
            rc = grow_parity_scratch(ctx, group, per_block);
        if (!rc && generated)  // the row pointers of the largest group: [group][k] then [group][e]
            rc = ensure_scratch(ctx, align_up(sizeof(void*) * (size_t)k * group, 256) +
                                         align_up(sizeof(void*) * (size_t)e * group, 256));
        // the matrix on the device (behind the update's tables)
        if (!rc)
            rc = update_tables(ctx, k, e, coef);
        if (rc)
            return rc;
        RS_HIP(ctx, hipMemsetAsync(d_report, 0, blocks * sizeof(rsgpu_scrub_report), ctx->stream));
    }
    for (size_t g0 = 0; g0 < blocks; g0 += group) {
        const size_t ng = std::min(group, blocks - g0);
        LocateArgs a{};
        a.k = k;
        a.e = e;
        a.u = u;
        a.work = work ? 1 : 0;
        a.pitch = (long long)pitch;
        a.len = (long long)len;
        a.blocks = (long long)ng;
        a.slots = slots;
        a.cand_stride = stride;
        a.rows = d_rows + g0 * (size_t)u;
        a.report = d_report + g0;
        if (work) {
            a.cand = (uint8_t*)ctx->locate.p;
            a.coef = (const uint8_t*)ctx->d_update + kUpdTabBytes;
            auto span = [&](size_t b0, size_t nb, const uint8_t* calc) {
                LocateArgs c = a;
                c.blocks = (long long)nb;
                c.cand = a.cand + (b0 - g0) * stride;
                c.report = d_report + b0;
                c.calc = calc;
                c.par = d_parity + b0 * per_block;
                auto launch = [&](bool bytes, long long c0, long long c1) {
                    return launch_locate_span(c, bytes, c0, c1, bytes ? gx_bytes : gx_vec, bytes ? (int)gx_vec : 0,
                                              ctx->stream);
                };
                return launch_head_and_tail(ctx, kLocateNames, nb, n16, (long long)len, launch);
            };
            // fused: the claims are counted in the reports' status field, zero since the memset
            a.claimed = fused ? 1 : 0;
            if (generated) {
                JitLocateArgs s{};
                s.fold = reinterpret_cast<ScrubFold*>(d_report + g0);
                s.cand = a.cand;
                s.cand_stride = stride;
                s.slots = slots;
                s.u = u;
                rc = generated_prepare(ctx, k, e, len, pitch, ng, d_src + g0 * (size_t)k * pitch,
                                       d_parity + g0 * per_block, matrix.data(), nullptr, s);
                if (!rc)
                    rc = generated_launch(ctx, s, ng, "k_rs_jit_locate", launch_rs_jit_locate);
                if (rc)
                    return rc;
            } else if (compiled) {
                KTimer kt(ctx, "k_rs_bs_locate", ng);
                RS_HIP(ctx, launch_rs_bitsliced_locate(k, e, d_src + g0 * (size_t)k * pitch,
                                                       d_parity + g0 * per_block, (long long)pitch, (long long)len,
                                                       (long long)ng, reinterpret_cast<ScrubFold*>(d_report + g0),
                                                       a.cand, stride, u, ctx->stream));
            } else {
                rc = two_pass(ctx, k, e, len, pitch, g0, ng, d_src, coef, nullptr, span);
                if (rc)
                    return rc;
            }
        }
        KTimer kt(ctx, "k_locate_finish", ng);
        RS_HIP(ctx, launch_locate_finish(a, ctx->stream));
    }
    return RSGPU_OK;
}

}  // extern "C"
