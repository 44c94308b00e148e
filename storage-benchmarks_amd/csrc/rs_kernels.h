// rs_kernels.h -- launch interface of the HIP kernels (internal to librsgpu).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct rsgpu_scrub_report;  // include/rsgpu.h

namespace rsgpu {

// Most kernels put the block index in grid.y (or z), whose limit is 65535:
// the block-batched entry points run larger batches as consecutive slices.
constexpr size_t kMaxGridBlocks = 65535;

struct DotArgs {
    const uint8_t* const* srcs;   // device [blocks][k] row pointers
    uint8_t* const* dsts;         // device [blocks][rows] row pointers
    const uint4* tabs4;           // device [blocks?][k][rows_pad] (perm tables, bits 0-5)
    const uint32_t* ctab;         // device [blocks?][k][rows_pad] (perm table, bits 6-7)
    long long tab_block_stride;   // coefficients between blocks' tables (0 = shared)
    int k, rows, rows_pad;
    long long len;                // bytes per row
    long long blocks;
    const int* status;            // optional [blocks]: skip blocks with status != 0
    bool bytewise;                // pointers not 8-byte aligned: byte kernel
};

// General decode preparation (k_decode_prepare, one workgroup per block):
// survivors = the first k rows of the m-row code not erased (ascending),
// their k x k matrix inverted (Gauss-Jordan, isa/ec_base.c:99-152), with the
// reference's retry when singular (erasure_code_base_test.c:163-184); decode
// rows = inverse rows of erased data rows, encode row x inverse for erased
// parity rows (:197-210).
struct PrepArgs {
    int k, m, nerrs, rows_pad;
    long long blocks;
    const uint8_t* err;           // device [blocks][nerrs], strictly ascending, < m
    const uint8_t* enc;           // device m x k encode matrix, nullptr = gf_gen_rs_matrix(m, k)
    int originals_only;           // isa_decoder form: every erased index must be < k
    const uint8_t* src; long long src_pitch;   // [blocks][k] rows
    const uint8_t* par; long long par_pitch;   // [blocks][m - k] rows
    uint8_t* out; long long out_pitch;         // [blocks][nerrs] rows
    const uint8_t** surv_ptrs;    // device [blocks][k]
    uint8_t** out_ptrs;           // device [blocks][nerrs]
    uint4* tabs4; uint32_t* ctab; long long tab_block_stride;  // v_perm tables, or nullptr
    int* status;                  // device [blocks]
    // k_rs_tc instead of k_dot_generic (when non-null): the context's
    // 2048-entry handler table and the address output, tc_block_stride
    // elements per block in the pass layout of tc_table_elems()
    const unsigned long long* tc_table = nullptr;
    unsigned long long* tc_addr = nullptr;
    long long tc_block_stride = 0;
    // or (when non-null) the decode rows themselves, [blocks][nerrs][k], for
    // k_jit_emit
    uint8_t* coef_out = nullptr;
};

int generic_rows_per_pass(int rows);
hipError_t launch_dot_generic(const DotArgs& a, hipStream_t st);
bool rs_encode_specialized_available(int k, int e);
hipError_t launch_rs_encode_specialized(int k, int e, const uint8_t* src, uint8_t* par,
                                        long long pitch, long long len, long long blocks,
                                        hipStream_t st);
size_t decode_prepare_lds_bytes(int k);
hipError_t launch_decode_prepare(const PrepArgs& a, hipStream_t st);
hipError_t launch_fill_synth(uint8_t* dst, long long rows, long long len, long long pitch,
                             unsigned long long seed, unsigned long long row0, hipStream_t st);
hipError_t launch_compare_rows(const uint8_t* src, long long src_pitch, int k, const uint8_t* out,
                               long long out_pitch, int e, const uint8_t* err, long long len,
                               long long blocks, unsigned long long* mismatches, hipStream_t st);
// Bit-sliced RS(k, e) parity of the gf_gen_rs_matrix code with compile-time
// coefficients (rs_bitsliced.hip).  Requires len % 32 == 0, 16-byte aligned
// rows.
bool rs_bitsliced_available(int k, int e);
// output rows each wave of the compiled kernel owns (its composites of a
// source are built per this many rows), 0 if none is compiled for (k, e)
int rs_bitsliced_rows_per_wave(int k, int e);
hipError_t launch_rs_bitsliced(int k, int e, const uint8_t* src, uint8_t* out, long long pitch,
                               long long len, long long blocks, hipStream_t st, int prio = 0);
// Small batches of the single-chunk codes (16,4) (16,8) (5,4) (20,7): four
// waves per tile split the sources (k_rs_bs_split), same bytes.
bool rs_bitsliced_split_available(int k, int e);
// small-batch decode of those codes in one launch: syndromes through the
// compiled programs, the e x e solve with runtime coefficients
struct SynArgs {
    const uint8_t* src;  // [B][k] rows (erased ones never read)
    const uint8_t* par;  // [B][e] rows
    uint8_t* out;        // [B][e] rows, ascending erased order
    const uint8_t* err;  // [B][e] erased originals, strictly ascending
    int* status;         // [B]
    long long pitch, len;
};
hipError_t launch_rs_syn_split(int k, int e, const SynArgs& a, long long blocks, hipStream_t st);
hipError_t launch_rs_bitsliced_split(int k, int e, const uint8_t* src, uint8_t* out, long long pitch,
                                     long long len, long long blocks, hipStream_t st);

// Parity scrub (rsgpu_scrub_blocks).  While a call is in flight a block's
// 16-byte report holds the fold of its tiles, every field zero at the start
// (one memset) and only ever raised by order-independent atomics:
//   bytes 0-7   bad columns so far (atomicAdd)
//   bytes 8-11  max over bad columns of row + 1          (kScrubNoRow when no
//   bytes 12-15 max over bad columns of kScrubBias - row   row explains one)
// so the block has one damaged row exactly when the two maxima name the same
// row; k_scrub_finalise turns the fold into (status, row).
constexpr unsigned kScrubBias = 1024;   // > any row index (k + e <= 250)
constexpr unsigned kScrubNoRow = 2000;  // > kScrubBias: never equal to a row's pair
struct ScrubFold {
    unsigned long long bad;
    unsigned hi1, lo1;
};
// Two-pass compare: the syndromes are calc ^ par (any alignment; 16 bytes per
// load when the rows allow); rowtab [256] maps the ratio s_1 / s_0 to a source row (255:
// none), coef is the e x k matrix (both device memory, read only with locate).
struct ScrubCmpArgs {
    static constexpr bool kRepair = false;  // scrub_column only reads
    const uint8_t* calc;  // [B][e] rows: the parity of the sources, recomputed
    const uint8_t* par;   // [B][e] rows: the stored parity
    long long pitch, len, blocks;
    int k, e;
    const uint8_t* rowtab;
    const uint8_t* coef;
    ScrubFold* fold;  // [B]
    int locate;
};
hipError_t launch_scrub_compare(const ScrubCmpArgs& a, hipStream_t st);
hipError_t launch_scrub_finalise(void* report, long long blocks, int locate, hipStream_t st);
// The fused scrub of the compiled codes (rs_bitsliced.hip k_rs_bs_scrub): the
// encode's accumulation, then the stored parity read and compared in
// registers.  len % 32 == 0, len < 2^32, 16-byte aligned rows, blocks <= 65535.
hipError_t launch_rs_bitsliced_scrub(int k, int e, const uint8_t* src, const uint8_t* par, long long pitch,
                                     long long len, long long blocks, ScrubFold* fold, int locate,
                                     hipStream_t st);

// Repair in place (rsgpu_repair_blocks): the scrub's kernels with writable
// rows, correcting the byte of a bad column where its row and error value are
// already at hand.  A block's 24-byte report holds its fold while a call is in
// flight (zeroed by one memset, as the scrub's):
//   bytes 0-7    bad columns (atomicAdd)
//   bytes 8-15   corrected columns (atomicAdd; COLUMNS only)
//   bytes 16-19  max of row + 1          over the columns that count for `row`:
//   bytes 20-23  max of kScrubBias - row   every bad one (ONE_ROW, kScrubNoRow
//                where no row explains it), the corrected ones (COLUMNS)
// k_repair_finalise turns it into the report.  The kernels run in one of
// three modes:
//   kRepairLocate   ONE_ROW pass 1: fold, write no row byte
//   kRepairGated    ONE_ROW pass 2, after the finalise: a workgroup whose
//                   block's report is not REPAIRED (bytes 16-19 != kRepairGate)
//                   leaves before it loads anything; the others correct and
//                   touch no report
//   kRepairColumns  COLUMNS: fold and correct in one pass
constexpr int kRepairLocate = 0, kRepairGated = 1, kRepairColumns = 2;
constexpr unsigned kRepairGate = 1;  // RSGPU_REPAIR_REPAIRED
struct RepairFold {
    unsigned long long bad, rep;
    unsigned hi1, lo1;
};
struct RepairCmpArgs {
    static constexpr bool kRepair = true;
    static constexpr int locate = 1;
    const uint8_t* calc;  // [B][e] rows: the parity of the sources, recomputed
    uint8_t* src;         // [B][k] rows
    uint8_t* par;         // [B][e] rows: the stored parity
    long long pitch, len, blocks;
    int k, e;
    const uint8_t* rowtab;
    const uint8_t* coef;
    RepairFold* fold;  // [B]
    int mode;
};
hipError_t launch_repair_compare(const RepairCmpArgs& a, hipStream_t st);
// mode: RSGPU_REPAIR_ONE_ROW / _COLUMNS
hipError_t launch_repair_finalise(void* report, long long blocks, int mode, hipStream_t st);
// k_rs_bs_repair: k_rs_bs_scrub's conditions
hipError_t launch_rs_bitsliced_repair(int k, int e, uint8_t* src, uint8_t* par, long long pitch, long long len,
                                      long long blocks, RepairFold* fold, int mode, hipStream_t st);

// Closed-form decode prepare for the gf_gen_rs_matrix code with e erased
// originals and all e parity rows surviving, per block: erasure list
// validation (strictly ascending, < k; else status -2), srcs [B][k] =
// surviving originals (ascending) then the e parity rows, dsts [B][e] = out
// rows, and the e x k decode rows V_E^-1 [V_kept | I] (no elimination) as
//   dir_addr != nullptr  k_rs_tc handler addresses [B][k][tc_rows_per_pass(e)]
//                        (e <= 32; tc_table = the context's handler table)
//   jit_coef != nullptr  the rows themselves, [B][e][k] bytes, which the
//                        emitters turn into k_rs_jit / k_rs_jitw code (e <= 63)
hipError_t launch_decode_prepare_syn(int k, int e, long long blocks, const uint8_t* err,
                                     uint8_t* out, long long out_pitch, const uint8_t** srcs,
                                     uint8_t** dsts, const unsigned long long* tc_table, int* status,
                                     const uint8_t* src, const uint8_t* par,
                                     unsigned long long* dir_addr, uint8_t* jit_coef, hipStream_t st);

// The one-matrix decode through generated code (rs_jit.hip).
struct JitArgs {
    const uint8_t* const* srcs;      // [B][k]
    uint8_t* const* dsts;            // [B][dst_stride], this launch's rows first
    const uint8_t* code;             // executable: block b, wave w, chunk ch at
                                     // code + b block_stride + (w nch + ch) chunk_stride
    long long chunk_stride;          // jit::chunk_stride(8), or jit::host_chunk_stride()
    long long block_stride;          // bytes; 0 = one program shared by every block
    int k, rows;                     // rows <= 32
    int dst_stride;                  // output pointers per block (>= rows)
    long long len;                   // % 32 == 0
    const int* status;               // [B] or nullptr (every block runs)
    int xcd_order;                   // non-zero: XCD-contiguous (block, tile) order
    int tiles_per_wg = 1;            // k_rs_jitw: column tiles per workgroup (1, 2 or 3)
    int code_prefetch = 0;           // k_rs_jitw: workgroups pull their block's code into L2 first
    int chunk_rot_ticks = 0;         // k_rs_jitw: > 0 rotates the chunk order by the start time
                                     // (s_memrealtime / chunk_rot_ticks), 0 = chunks in order
    int prio = 0;                    // k_rs_jitw / k_rs_jit: wave priority from transposes to barrier
};
// k_rs_jitw's chunk rotation period for `rows` rows at k sources: about one
// chunk's duration in 100 MHz ticks (measured best at 600 for C3's 16 rows)
int jitw_rot_ticks(int rows);
size_t jit_code_bytes(int k, int e, long long blocks);
// k_rs_jit's straight-line code (rs_jit.h) for every (block, wave, chunk) at
// code + ((b NW + w) nch + ch) jit::chunk_stride(8), from the decode rows
// coef [B][e][k] (k_decode_prepare_syn); blocks with status != 0 skipped.
hipError_t launch_jit_emit(int k, int e, long long blocks, const uint8_t* coef, const int* status,
                           uint8_t* code, hipStream_t st);
hipError_t launch_jit_fill(void* code, size_t bytes, hipStream_t st);
hipError_t launch_rs_jit(const JitArgs& a, long long blocks, hipStream_t st);
// Two waves of R rows per tile (rs_jit.h Wide): R = jitw_rows(e) (16 for
// 24 < e <= 32, 12 for 20 < e <= 24, 10 for 16 < e <= 20, else 0 = not this
// layout); code of
// block b, wave w, chunk ch at code + ((b 2 + w) nch + ch) jitw_chunk_stride(e)
int jitw_rows(int e);
// sources per chunk of that layout (rs_jit.h Wide<R, CS>)
int jitw_cs(int e);
size_t jitw_chunk_stride(int e);
size_t jitw_code_bytes(int k, int e, long long blocks);
// the wide layout covers e (16 < e <= 64 one launch; 64 < e <= 125 in passes
// of <= 64 rows, rs_jit.h wide_passes), and a pass's place in a block's code
bool jitw_layout(int e);
size_t jitw_pass_bytes(int k, int rows);
size_t jitw_pass_offset(int k, int e, int p);
hipError_t launch_jitw_emit(int k, int e, long long blocks, const uint8_t* coef, const int* status,
                            uint8_t* code, hipStream_t st);
hipError_t launch_rs_jitw(const JitArgs& a, long long blocks, hipStream_t st);
// The (64, 32) gf_gen_rs_matrix encode through the Karatsuba-split program
// (jit_prog.h build_karatsuba_code; k_rs_kara): a.code / a.chunk_stride the
// program, a.k = 64, a.rows = 32, one column tile per workgroup, chunk_rot_ticks
// and prio as k_rs_jitw.
hipError_t launch_rs_kara(const JitArgs& a, long long blocks, hipStream_t st);
// rsgpu_ec_encode_data_batch: blocks of their own rows and lengths, at most
// kMaxGridBlocks per launch.  k_ec_batch_classify (one wave per block) reads
// len[b] and, unless it is 0, the block's k + rows pointers, and writes
//   status[b] (when given)  0, or -2 for a block the call rejects: len[b] < 0
//              or > max_len, and under `aligned32` a length that is no
//              multiple of 32 or a pointer that is not 16-byte aligned
//   lo[b]      where the block's byte range starts: len[b] & ~31 when every
//              pointer is 16-byte aligned and `fast` is set, else 0
//   end[b]     len[b], or 0 for a rejected block
struct BatchClassifyArgs {
    const uint8_t* const* srcs;  // [B][k]
    uint8_t* const* dsts;        // [B][rows]
    const int* len;              // [B]
    int k, rows, max_len;
    int aligned32, fast;
    long long blocks;
    int* status;                 // [B] or nullptr
    int* lo;                     // [B]
    int* end;                    // [B]
};
hipError_t launch_ec_batch_classify(const BatchClassifyArgs& a, hipStream_t st);
// The shared program of launch_rs_jit (rows <= 32, a.block_stride == 0) or,
// with `wide`, of launch_rs_jitw over [0, lo[b]) of every block b: the grid covers max_lo
// bytes (% 32 == 0, the host's bound of every lo[b]), and a workgroup whose
// first tile starts at or behind lo[b] leaves before it touches a pointer or
// LDS.  a.len and a.status are not used.
hipError_t launch_rs_jit_batch(const JitArgs& a, bool wide, const int* lo, long long max_lo, long long blocks,
                               hipStream_t st);
// k_dot_bytes with one table for every block (DotArgs::tab_block_stride == 0)
// over bytes [first[b], end[b]) of block b; a.len is the host's bound of every
// end[b] and sizes the grid.  a.status and a.bytewise are not used.
hipError_t launch_dot_bytes_batch(const DotArgs& a, const int* first, const int* end, hipStream_t st);
// The generated scrub (k_rs_jit_scrub, k_rs_jitw_scrub): the shared program's
// accumulation exactly as the encode runs it, then the stored parity rows read
// through j.dsts (never written) and compared in registers.  j.rows = e <= 64
// in one launch, j.block_stride == 0, j.status == nullptr, j.len < 2^32; the
// fold zeroed before the launch; tab (read only with locate): [rowtab 256 B |
// e x k matrix], the head of the two-pass scratch.
struct JitScrubArgs {
    JitArgs j;
    ScrubFold* fold;     // [B]
    const uint8_t* tab;
    int locate;
};
hipError_t launch_rs_jit_scrub(const JitScrubArgs& a, long long blocks, hipStream_t st);
// The generated locate (k_rs_jit_locate, k_rs_jitw_locate; rsgpu_locate_blocks
// under FUSED with the scrub kernel GENERATED): the generated scrub up to the
// count of bad columns, then k_rs_bs_locate's contract (below, at
// launch_rs_bitsliced_locate) for any matrix: a workgroup with a bad column
// reduces the syndrome columns of all its tiles to a basis of at most u
// vectors and writes it to the slot it claims with an atomicAdd on fold[b].hi1
// (zero before the launch).  A block's area holds `slots` slots, one per tile
// of 2048 bytes; a workgroup covers at least one tile and claims at most one
// slot.  k_locate_finish with `claimed` follows.  j as JitScrubArgs::j; 1 <= u
// <= 8.
struct JitLocateArgs {
    JitArgs j;
    ScrubFold* fold;     // [B]; hi1 counts the block's claimed slots
    uint8_t* cand;       // [B] candidate areas at cand_stride
    size_t cand_stride;
    int slots;           // per block
    int u;
};
hipError_t launch_rs_jit_locate(const JitLocateArgs& a, long long blocks, hipStream_t st);
// The generated repair (k_rs_jit_repair, k_rs_jitw_repair; rsgpu_repair_blocks
// under RSGPU_REPAIR_KERNEL_GENERATED): the generated scrub with locate, on the
// 24-byte fold, correcting in its cold path in one of the three modes above (at
// RepairFold).  j as JitScrubArgs::j; src and par: the writable rows that
// j.srcs and j.dsts name, block b's at src + b k pitch and par + b e pitch;
// tab as JitScrubArgs::tab, of a locatable matrix.
struct JitRepairArgs {
    JitArgs j;
    RepairFold* fold;  // [B]: zeroed (kRepairLocate, kRepairColumns) or the final reports (kRepairGated)
    const uint8_t* tab;
    int mode;
    uint8_t* src;
    uint8_t* par;
    long long pitch;
};
hipError_t launch_rs_jit_repair(const JitRepairArgs& a, long long blocks, hipStream_t st);
// The generated correction (k_rs_jit_correct, k_rs_jitw_correct;
// rsgpu_correct_blocks under RSGPU_CORRECT_FUSED with the scrub kernel
// GENERATED): the generated repair in its kRepairColumns mode on the 32-byte
// fold (CorrectFold, below), whose cold path, with t == 2, searches the row
// pairs for every bad column no single row explains (rs_correct.hip's search
// for a matrix read from memory, rs_pairs.h pair_search_lane).  j, src, par,
// pitch and tab as JitRepairArgs'; t as CorrectCmpArgs'.  The search keeps its
// tables in the chunk buffers; jit_correct_fits says whether they fit for
// (k, e, t) -- t == 1 always, t == 2 everywhere but at 60 <= e <= 64 with
// 256 e + 32 k > 21240 -- and the launch refuses where they do not.
struct CorrectFold;
struct JitCorrectArgs {
    JitArgs j;
    CorrectFold* fold;  // [B], zeroed before the launch
    const uint8_t* tab;
    int t;
    uint8_t* src;
    uint8_t* par;
    long long pitch;
};
bool jit_correct_fits(int k, int e, int t);
hipError_t launch_rs_jit_correct(const JitCorrectArgs& a, long long blocks, hipStream_t st);
// small uploads through the kernel arguments (k_put_words): bytes % 8 == 0,
// at most sizeof(PutArgs::w)
struct PutArgs {
    static constexpr int kWords = 128;
    uint64_t w[kWords];
    uint64_t* dst;
    int n;
};
hipError_t launch_put_words(void* dst, const void* src, size_t bytes, hipStream_t st);
// device-to-device copy into executable memory (host-built code staged in
// ordinary device memory first), bytes % 8 == 0
hipError_t launch_jit_copy(void* dst, const void* src, size_t bytes, hipStream_t st);

// Threaded-code bit-sliced dot product with runtime coefficients (rs_tc.hip):
// dsts[b][i] = sum_p c_b[i][p] * srcs[b][p] for rows <= 32 per launch, where
// the coefficients arrive as handler addresses addr[b][p][slot] (slot <
// tc_rows_per_pass(rows), padding slots point at handler 0).  len % 32 == 0,
// 16-byte aligned rows; blocks with status != 0 are skipped.  More than 32
// rows run as passes of 32 (the address tables in the pass layout below).
struct TcArgs {
    const uint8_t* const* srcs;      // [B][k]
    uint8_t* const* dsts;            // [B][dst_stride], this launch's rows first
    int dst_stride;                  // row pointers per block in dsts
    const unsigned long long* addr;  // [B][k][tc_rows_per_pass(rows)]
    long long addr_stride;           // elements between blocks' tables (0: shared)
    int k, rows;
    long long len;
    const int* status;               // [B] or nullptr
};
// slots of a pass of rows <= 32: rows rounded up to 8
__host__ __device__ inline int tc_rows_per_pass(int rows) { return rows <= 0 ? 8 : (rows + 7) / 8 * 8; }
// Pass layout of a handler-address table for `rows` output rows over k
// sources: pass p (rows 32p .. 32p+31) at element offset tc_pass_offset,
// [k][tc_rows_per_pass(pass rows)] each; tc_table_elems in total.
__host__ __device__ inline int tc_passes(int rows) { return rows <= 0 ? 1 : (rows + 31) / 32; }
__host__ __device__ inline int tc_pass_rows(int rows, int p) { return rows - 32 * p < 32 ? rows - 32 * p : 32; }
__host__ __device__ inline long long tc_pass_offset(int k, int p) { return (long long)k * 32 * p; }
__host__ __device__ inline long long tc_table_elems(int k, int rows)
{
    const int np = tc_passes(rows);
    return tc_pass_offset(k, np - 1) + (long long)k * tc_rows_per_pass(tc_pass_rows(rows, np - 1));
}
// element of (output row r, source j) in a pass-layout table
__host__ __device__ inline long long tc_elem(int k, int rows, int r, int j)
{
    const int p = r / 32;
    return tc_pass_offset(k, p) + (long long)j * tc_rows_per_pass(tc_pass_rows(rows, p)) + (r & 31);
}

int tc_handler_stride();
// handlers in the table (256 per handler copy of the chained dispatch) and
// the copy serving slot s (0..7).  Consumers index the context's 2048-entry
// address table as tc_table[(slot & 7) * 256 + c]: the address of handler
// (tc_slot_copy(slot), c).
int tc_handler_count();
int tc_slot_copy(int slot);
hipError_t tc_query_handlers(unsigned long long* d_out, hipStream_t st);
hipError_t launch_rs_tc(const TcArgs& a, long long blocks, hipStream_t st);
// The same for small batches with rows <= 8 (k >= 4): four waves per tile
// split the sources, partial accumulators reduced in LDS (rs_tc.hip
// k_rs_tc_split); addr [B][k][8] as above.
hipError_t launch_rs_tc_split(const TcArgs& a, long long blocks, hipStream_t st);
// The whole one-matrix decode of a small batch in one launch (rs_tc.hip
// k_rs_tc_fused): e <= 8, 1 <= k <= 64, len % 32 == 0, 16-byte aligned rows;
// the closed-form decode rows of every block built in the kernel, status
// written per block (0, or -2 for a malformed erasure list).
struct TcFusedArgs {
    int k, e;
    long long len, pitch, blocks;
    const uint8_t* err;      // [B][e] erased originals, strictly ascending
    const uint8_t* src;      // [B][k] rows (erased ones never read)
    const uint8_t* par;      // [B][e] rows
    uint8_t* out;            // [B][e] rows
    int* status;             // [B]
    // handler of (slot s, coefficient c): map_base + (map_copy[s] 256 + c) map_stride
    unsigned long long map_base;
    int map_stride;
    int map_copy[8];
};
hipError_t launch_rs_tc_fused(const TcFusedArgs& a, hipStream_t st);

hipError_t launch_row_ptrs(const uint8_t* base, long long pitch, int rows_per_block,
                           long long blocks, const uint8_t** out, hipStream_t st);
hipError_t launch_update(const uint8_t* data, uint8_t* const* coding, const uint4* tabs4,
                         const uint32_t* ctab, int rows, long long len, hipStream_t st);

// The column kernels of update, degraded scrub and rebuild are instantiated
// for G = 1, 2, 4 or 8 rows held per lane and clamp a block's count to G
// (`nout < G ? nout : G`), so G must cover the most rows any block of the call
// can have.  This is that rule, for the launchers and for RebuildArgs::g.
inline int lane_group(int most) { return most > 4 ? 8 : most > 2 ? 4 : most > 1 ? 2 : 1; }

// Partial-stripe update (rsgpu_update_blocks, rs_update.hip k_update_blocks):
// per block the rows its list names are replaced (or taken as deltas) and the
// e parity rows follow, parity[p] ^= XOR_i c[p][j_i] * delta_i.  blocks <=
// 65535 per launch.
struct UpdateArgs {
    int k, e, u;
    int delta;            // non-zero: upd rows are deltas, src is not touched
    long long pitch, blocks;
    const uint8_t* cols;  // [B][u] listed rows, ascending, then RSGPU_UPDATE_NONE
    const uint8_t* upd;   // [B][u] rows
    uint8_t* src;         // [B][k] rows (unused with delta)
    uint8_t* par;         // [B][e] rows
    const uint8_t* coef;  // device e x k matrix
    const uint4* tab4;    // device [256]: perm_tables words 0-3 of every coefficient value
    const uint32_t* tabc; // device [256]: perm_tables word 4
    int* status;          // [B]: 0, or -2 for a malformed list (block untouched)
};
// rows of a list one walk over the parity serves (the in-register group)
int update_group_rows();
// bytes == false: columns [col0, col1) are 16-byte units of 16-byte aligned
// rows; bytes == true: byte columns, any alignment.  An empty range only
// validates the lists and writes the statuses.
hipError_t launch_update_blocks(const UpdateArgs& a, bool bytes, long long col0, long long col1, hipStream_t st);

// Degraded scrub (rsgpu_scrub_degraded_blocks, rs_degraded.hip): blocks with
// known-lost rows.  k_degraded_prepare writes one table per block,
//   [DegradedHdr | rest: degraded_rest_bytes(e) | R: e x 8 | H: (k + e) x e]
// at degraded_tab_stride(k, e): the pivot parity rows Q (one per lost data
// row), the other surviving parity rows `rest`, R[pi][i] = the factor of pivot
// syndrome i in the reduced syndrome of rest row pi, and (locate only) H[r] =
// the reduced column of row r, zero for a lost row.  state != kDegRun: the
// prepare has written the block's final report and the compare and the
// finalise leave it alone.  The compare folds into the report's own 16 bytes
// as the scrub does (a ScrubFold, with its constants kScrubBias and
// kScrubNoRow).
constexpr int kDegRun = 0;      // the compare runs; the report holds a zeroed fold
constexpr int kDegClean = 100;  // e == 0 or len == 0 with a well-formed list: CLEAN
// any other state is the block's status: UNCHECKED, BAD_MATRIX or BAD_LIST
struct DegradedHdr {
    int state;
    uint8_t nq, nrest, pad[2];
    uint8_t q[8];  // parity indices p < e of the pivot rows, ascending
};
struct DegradedArgs {
    int k, e, u;
    int locate;
    int work;  // 0: e == 0 or len == 0, only the lists are judged
    long long pitch, len, blocks;
    const uint8_t* lost;   // [B][u]
    const uint8_t* coef;   // device e x k matrix
    const uint8_t* calc;   // [B][e] rows: the parity of the sources as stored, recomputed
    const uint8_t* par;    // [B][e] rows: the stored parity
    uint8_t* tab;          // [B] tables at tab_stride
    size_t tab_stride, rest_bytes;
    const uint4* tab4;     // device [256]: perm_tables words 0-3 of every coefficient value
    const uint32_t* tabc;  // device [256]: perm_tables word 4
    ::rsgpu_scrub_report* report;  // [B]
};
// (constant expressions: k_rs_bs_degraded takes them from its template arguments)
constexpr size_t degraded_rest_bytes(int e) { return ((size_t)e + 15) / 16 * 16; }
constexpr size_t degraded_tab_stride(int k, int e)
{
    return (sizeof(DegradedHdr) + degraded_rest_bytes(e) + (size_t)e * 8 + (size_t)(k + e) * e + 15) / 16 * 16;
}
hipError_t launch_degraded_prepare(const DegradedArgs& a, hipStream_t st);
// bytes == false: columns [col0, col1) are 16-byte units of 16-byte aligned
// rows; bytes == true: byte columns, any alignment
hipError_t launch_degraded_compare(const DegradedArgs& a, bool bytes, long long col0, long long col1,
                                   hipStream_t st);
hipError_t launch_degraded_finalise(const DegradedArgs& a, hipStream_t st);
// The degraded scrub fused into the compiled encode (rs_bitsliced.hip
// k_rs_bs_degraded), between the prepare and the finalise in place of the
// encode and the compare: the accumulation of k_rs_bs_scrub, then the
// syndromes reduced with the block's table and compared in registers; `fold`
// is the blocks' reports.  The fused scrub's geometry (len % 32 == 0, len <
// 2^32, 16-byte aligned rows, blocks <= 65535); `tab`: the blocks' tables at
// degraded_tab_stride(k, e), 16-byte aligned.  A lost parity row is never read.
hipError_t launch_rs_bitsliced_degraded(int k, int e, const uint8_t* src, const uint8_t* par, long long pitch,
                                        long long len, long long blocks, const uint8_t* tab, ScrubFold* fold,
                                        int locate, hipStream_t st);

// The degraded scrub fused into the matrix's generated encode (rs_jit.hip
// k_rs_jit_degraded, k_rs_jitw_degraded; FUSED with the scrub kernel
// GENERATED), in the same place: the shared program's accumulation exactly as
// the GENERATED encode and scrub run it, then the syndromes reduced with the
// block's table and compared in registers, for any matrix.  j as
// JitScrubArgs::j (j.rows = e <= 64); tab and fold as
// launch_rs_bitsliced_degraded's, tab_stride >= degraded_tab_stride(k, e) and a
// multiple of 16.  A lost parity row is never read.
struct JitDegradedArgs {
    JitArgs j;
    const uint8_t* tab;
    size_t tab_stride;
    ScrubFold* fold;  // [B]
    int locate;
};
hipError_t launch_rs_jit_degraded(const JitDegradedArgs& a, long long blocks, hipStream_t st);

// Rebuild in place (rsgpu_rebuild_blocks, rs_rebuild.hip): the listed rows of
// a block, and with `check` the one row its degraded report names, written
// back as fixed linear combinations of k surviving rows: the surviving data
// rows and the |D| pivot parity rows.  k_rebuild_prepare writes one table per
// block,
//   [RebuildHdr | sources: rebuild_src_bytes(k) | M: k x 8]
// at rebuild_tab_stride(k): the k source rows (indices in [0, k + e)), the
// rows to write, and M[s][o] = the factor of source s in output o.  state !=
// kRebRun: nothing of the block is written, and its report is final.
constexpr int kRebRun = 0;
constexpr int kRebStop = 1;
struct RebuildHdr {
    int state;
    uint8_t nout, pad[3];
    uint8_t out[8];  // rows in [0, k + e) to write, ascending
};
struct RebuildArgs {
    int k, e, u;
    int check;  // non-zero: report holds the degraded scrub's verdict (with locate) of every block
    int work;   // 0: e == 0 or len == 0, only the lists are judged
    long long pitch, len, blocks;
    const uint8_t* lost;   // [B][u]
    const uint8_t* coef;   // device e x k matrix
    uint8_t* src;          // [B][k] rows
    uint8_t* par;          // [B][e] rows
    uint8_t* tab;          // [B] tables at tab_stride
    size_t tab_stride, src_bytes;
    int g;                 // outputs a lane holds: lane_group(most rows of any block's list)
    const uint4* tab4;     // device [256]: perm_tables words 0-3 of every coefficient value
    const uint32_t* tabc;  // device [256]: perm_tables word 4
    ::rsgpu_scrub_report* report;  // [B]
};
size_t rebuild_src_bytes(int k);
size_t rebuild_tab_stride(int k);
hipError_t launch_rebuild_prepare(const RebuildArgs& a, hipStream_t st);
// bytes == false: columns [col0, col1) are 16-byte units of 16-byte aligned
// rows; bytes == true: byte columns, any alignment
hipError_t launch_rebuild_blocks(const RebuildArgs& a, bool bytes, long long col0, long long col1, hipStream_t st);

// Lists of up to RSGPU_REBUILD_MAX_LOST rows (k_rebuild_wide_prepare): the
// list judged, the verdict taken, Q chosen and c[Q][D] inverted as
// k_rebuild_prepare does, the elimination spread over the wave, and the k x n
// matrix of factors M formed by the same formulas.  Per block it writes
//   passes > 0  `passes` consecutive tables in k_rebuild_prepare's layout at
//               r.tab + b r.tab_stride (r.tab_stride >= passes x
//               rebuild_tab_stride(k)): table p serves outputs [8 p, 8 p + 8)
//               and has state != kRebRun when the block has none of them, so
//               k_rebuild_blocks runs once per pass with r.tab advanced
//   slots > 0   k_rs_tc's inputs: srcs [B][k] the source rows, dsts [B][slots]
//               the rows to write (null beyond the block's n), addr
//               [B][k][slots] = tc_table[(o & 7) * 256 + M[s][o]] with padding
//               slots at handler 0, and count [B] = n, 0 for a block that is
//               not rebuilt (its srcs, dsts and addr are then not written)
// slots = tc_rows_per_pass(most), most = min(u + check, e) <= 32.
struct RebuildWideArgs {
    RebuildArgs r;  // g unused
    int passes, slots;
    const unsigned long long* tc_table;  // the context's handler addresses [8][256]
    const uint8_t** srcs;
    uint8_t** dsts;
    unsigned long long* addr;
    int* count;
};
hipError_t launch_rebuild_wide_prepare(const RebuildWideArgs& a, hipStream_t st);
// k_rs_tc with a row count per block: a.status[b] (required) is the number of
// rows of block b to write, 0 skipping the block; a.rows, the most any block
// has, chooses the waves.  Rows are written where dsts says: in place is safe
// as long as no destination row is a source.
hipError_t launch_rs_tc_counted(const TcArgs& a, long long blocks, hipStream_t st);

// Locate several damaged rows per block (rsgpu_locate_blocks, rs_locate.hip).
// k_locate_span compares stored with recomputed parity as the scrub does and
// keeps, per workgroup, an echelon basis of the span of the syndrome columns
// it met: workgroup x of block b writes slot slot0 + x of the block's `slots`
// slots in the candidate area,
//   [n, overflow, 8 bytes unused | n <= u vectors of 64 bytes]
// at kLocateSlotBytes, and adds its bad columns to the report's first 8 bytes
// (zeroed before the first launch, as the scrub's fold).  Every slot of a
// block is written by exactly one workgroup of one launch before
// k_locate_finish (one wave per block) merges them, finds the rows whose
// column lies in the span and writes the list rows[b][u] and the report.
// (`claimed`, the fused form below: only the first report[b].hi1 slots are
// written, each by the workgroup that claimed it, and only they are read.)
constexpr size_t kLocateSlotBytes = 16 + 8 * 64;
struct LocateArgs {
    int k, e, u;
    int work;  // 0: e == 0 or len == 0, the finish reports every block CLEAN
    long long pitch, len, blocks;
    const uint8_t* calc;   // [B][e] rows: the parity of the sources, recomputed
    const uint8_t* par;    // [B][e] rows: the stored parity
    const uint8_t* coef;   // device e x k matrix (the finish)
    uint8_t* cand;         // [B] candidate areas at cand_stride
    size_t cand_stride;
    int slots;             // per block
    int claimed;           // non-zero: the first report[b].hi1 slots are written, no other (k_rs_bs_locate)
    uint8_t* rows;         // [B][u] (the finish)
    ::rsgpu_scrub_report* report;  // [B]
};
// bytes == false: columns [col0, col1) are 16-byte units of 16-byte aligned
// rows; bytes == true: byte columns, any alignment.  gx workgroups per block,
// writing slots [slot0, slot0 + gx).  e <= 64.
hipError_t launch_locate_span(const LocateArgs& a, bool bytes, long long col0, long long col1, unsigned gx, int slot0,
                              hipStream_t st);
hipError_t launch_locate_finish(const LocateArgs& a, hipStream_t st);
// The locate of the compiled codes fused into the encode (rs_bitsliced.hip
// k_rs_bs_locate): k_rs_bs_scrub's accumulation and compare; a workgroup whose
// tile has a bad column adds the count to fold[b].bad, reduces the tile's
// syndrome columns to a basis of at most u vectors and writes it to the slot
// it claims with an atomicAdd on fold[b].hi1 (zero before the launch): slot i
// of block b at cand + b * cand_stride + i * kLocateSlotBytes, one per tile of
// 2048 bytes at the most.  A clean tile writes nothing.  k_locate_finish with
// `claimed` follows.  The scrub's conditions on the rows; 1 <= u <= 8.
hipError_t launch_rs_bitsliced_locate(int k, int e, const uint8_t* src, const uint8_t* par, long long pitch,
                                      long long len, long long blocks, ScrubFold* fold, uint8_t* cand,
                                      size_t cand_stride, int u, hipStream_t st);

// Correction per byte column of up to t rows (rsgpu_correct_blocks,
// rs_correct.hip): k_repair_compare in its COLUMNS mode whose waves, with t ==
// 2, search the row pairs for every bad column no single row explains.  A
// block's 32-byte report holds its fold while a call is in flight (zeroed by
// one memset, as the repair's):
//   bytes 0-7    bad columns (atomicAdd)
//   bytes 8-15   corrected columns, one- and two-row together (atomicAdd)
//   bytes 16-23  of those, the columns corrected in two rows (atomicAdd)
//   bytes 24-27  max of row + 1          over the corrected columns, a two-row
//   bytes 28-31  max of kScrubBias - row   correction counting as kScrubNoRow
// k_correct_finalise turns it into the report.
struct CorrectFold {
    unsigned long long bad, rep, two;
    unsigned hi1, lo1;
};
struct CorrectCmpArgs {
    const uint8_t* calc;  // [B][e] rows: the parity of the sources, recomputed
    uint8_t* src;         // [B][k] rows
    uint8_t* par;         // [B][e] rows: the stored parity
    long long pitch, len, blocks;
    int k, e;
    const uint8_t* rowtab;  // as ScrubCmpArgs'
    const uint8_t* coef;
    CorrectFold* fold;  // [B]
    int t;              // 1: e >= 3; 2: 5 <= e <= 64
};
hipError_t launch_correct_compare(const CorrectCmpArgs& a, hipStream_t st);
hipError_t launch_correct_finalise(void* report, long long blocks, hipStream_t st);
// k_rs_bs_correct: k_rs_bs_scrub's conditions; the fold zeroed, launch_correct_finalise
// after the last slice.  t as CorrectCmpArgs'.
hipError_t launch_rs_bitsliced_correct(int k, int e, uint8_t* src, uint8_t* par, long long pitch, long long len,
                                       long long blocks, CorrectFold* fold, int t, hipStream_t st);

}  // namespace rsgpu
