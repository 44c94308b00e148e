/*
 * rsgpu.h -- C ABI of the MI355X-native Reed-Solomon GF(2^8) erasure engine
 * (librsgpu.so).  Drop-in boundary for the hot path of
 * steinwurf/storage-benchmarks' benchmark/isa_throughput: the plugin calls
 * the ISA-L 2.13 C ABI (isa-l_open_src_2.13/isa/erasure_code.h) from
 * isa_encoder::encode_all (benchmark/isa_throughput/isa.cpp:69-79) and
 * isa_decoder::decode_all (isa.cpp:169-213).  Every entry point below names
 * the reference interface it replaces.
 *
 * Conventions (same as the ISA-L ABI):
 *   - plain pointers and sizes, C linkage, no exceptions, no allocation of
 *     caller data: the caller owns every buffer (host or device);
 *   - status returns: RSGPU_OK (0) or a negative RSGPU_ERR_* code; the
 *     context keeps a message for rsgpu_last_error();
 *   - work is enqueued on the context's HIP stream (hipStream_t passed as
 *     void*); nothing synchronises unless the function says so.  Two waits
 *     belong to every call: the first use of a matrix (its generated program
 *     is built then) and a growth of a context-owned buffer may drain the
 *     stream; and host arguments (coef, gftbls, encode_matrix, pointer arrays)
 *     are read before the call returns and go through ONE pinned staging
 *     buffer per context, so a call that stages waits on the host until the
 *     context's previous staged upload has left that buffer -- at once when
 *     the stream is idle, and twice within a first use that uploads a program
 *     and a table (tests/test_gpu_stream_order.py lists the calls seen to);
 *   - one context per device and host thread; distinct contexts are
 *     independent (one process or thread per GPU).
 *
 * Device data layout of the batched calls ("blocks"): row r of block b of a
 * buffer with R rows per block lives at base + (b*R + r)*pitch, pitch >= len.
 * Source rows are the k original symbols, parity rows the e = m-k coded
 * symbols (gf_gen_rs_matrix rows k..m-1), exactly as isa_encoder's m_buffs
 * (isa.cpp:46-58) but contiguous in HBM.
 */
#ifndef RSGPU_H
#define RSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSGPU_OK 0
#define RSGPU_ERR_ARG (-1)
#define RSGPU_ERR_HIP (-2)
#define RSGPU_ERR_SINGULAR (-3)
#define RSGPU_ERR_NOMEM (-4)
#define RSGPU_ERR_UNSUPPORTED (-5)

#define RSGPU_MAX_SOURCES 250 /* TEST_SOURCES, isa.cpp:25-27 */

/* The longest row of every block-batched call below (the `size_t len` of
 * rsgpu_encode_blocks, rsgpu_decode_blocks, rsgpu_decode_prepare / _apply,
 * rsgpu_decode_general, rsgpu_verify_blocks, the scrub family, rsgpu_update_blocks
 * and the two host-resident calls): the kernels of 32-byte lanes add a 32-bit
 * byte offset to a 64-bit row address.  A longer len is refused with RSGPU_ERR_ARG and an
 * rsgpu_last_error text before anything is enqueued or written; a caller
 * with longer rows splits them into column ranges (advance d_src, d_parity
 * and the other row buffers by the range's start, keep the pitch).  pitch,
 * blocks and the buffers' total size have no such limit: every row address
 * is computed in 64 bits. */
#define RSGPU_MAX_LEN 0xFFFFFFFFull

typedef struct rsgpu_ctx rsgpu_ctx;

/* ---- version / context -------------------------------------------------- */

/* "major.minor.patch" of the engine */
const char *rsgpu_version(void);

/* Binds the calling thread to HIP device `device` and creates a context whose
 * stream is the device's null stream until rsgpu_set_stream(). */
int rsgpu_create(int device, rsgpu_ctx **out);
int rsgpu_destroy(rsgpu_ctx *ctx);
/* Moves the context to another stream.  Work already enqueued on the old
 * stream is ordered before anything the context enqueues afterwards (the new
 * stream waits on an event recorded on the old one): the context's internal
 * scratch and staging buffers are never reused while an earlier kernel may
 * still read them. */
int rsgpu_set_stream(rsgpu_ctx *ctx, void *hip_stream);
void *rsgpu_get_stream(rsgpu_ctx *ctx);
int rsgpu_synchronize(rsgpu_ctx *ctx);
const char *rsgpu_last_error(rsgpu_ctx *ctx);

/* Per-kernel timing (instrumentation, off by default): while enabled every
 * kernel the engine enqueues is bracketed by HIP events on the stream it runs
 * on.  rsgpu_timing_read() synchronises the streams, writes up to `max`
 * (kernel name, milliseconds, blocks processed) records in launch order
 * (any output array may be NULL), returns how many, and
 * clears the log.  Names are static strings owned by the library. */
int rsgpu_timing_enable(rsgpu_ctx *ctx, int on);
int rsgpu_timing_read(rsgpu_ctx *ctx, const char **names, float *ms, size_t *blocks,
                      int max);

/* Device memory helpers for C/C++ callers without another allocator. */
int rsgpu_malloc(rsgpu_ctx *ctx, void **dptr, size_t bytes);
int rsgpu_free(rsgpu_ctx *ctx, void *dptr);
int rsgpu_memcpy_h2d(rsgpu_ctx *ctx, void *dst, const void *src, size_t bytes);
int rsgpu_memcpy_d2h(rsgpu_ctx *ctx, void *dst, const void *src, size_t bytes);

/* ---- host GF(2^8) helpers: the ISA-L C ABI, same arguments/semantics ----- */

/* erasure_code.h gf_mul / gf_inv (isa/ec_base.c:36-60) */
unsigned char rsgpu_gf_mul(unsigned char a, unsigned char b);
unsigned char rsgpu_gf_inv(unsigned char a);
/* erasure_code.h:898 gf_gen_rs_matrix (isa/ec_base.c:62-79) */
void rsgpu_gf_gen_rs_matrix(unsigned char *a, int m, int k);
/* erasure_code.h gf_gen_cauchy1_matrix (isa/ec_base.c:81-97) */
void rsgpu_gf_gen_cauchy1_matrix(unsigned char *a, int m, int k);
/* erasure_code.h:924 gf_invert_matrix (isa/ec_base.c:99-152): destroys `in`,
 * returns 0 or -1 when singular. */
int rsgpu_gf_invert_matrix(unsigned char *in, unsigned char *out, const int n);
/* erasure_code.h gf_vect_mul_init (isa/ec_base.c:157-262): 32-byte table */
void rsgpu_gf_vect_mul_init(unsigned char c, unsigned char *tbl);
/* erasure_code.h:74 ec_init_tables (isa/ec_highlevel_func.c:33-43) */
void rsgpu_ec_init_tables(int k, int rows, unsigned char *a, unsigned char *gftbls);

/* ---- device, ISA-L-shaped ------------------------------------------------ */

/* erasure_code.h:98 ec_encode_data (isa/ec_multibinary.asm:112-162 dispatch,
 * isa/ec_highlevel_func.c:106-135 avx2 split): coding[r][i] =
 * XOR_j c[r][j]*data[j][i].  `gftbls` is HOST memory in ISA-L's 32-byte table
 * format (as produced by ec_init_tables); `data` / `coding` are HOST arrays
 * of DEVICE pointers; any len >= 0 and any alignment.
 *
 * This and the other pointer calls below write bytes [0, len) of each output
 * row (coding[r], dest) and nothing else: no byte before or behind a row, and
 * never any byte of data[j] / src. */
int rsgpu_ec_encode_data(rsgpu_ctx *ctx, int len, int k, int rows, const unsigned char *gftbls,
                         unsigned char **data, unsigned char **coding);

/* erasure_code.h ec_encode_data_update (isa/ec_highlevel_func.c:139-252,
 * isa/ec_base.c:307-321): coding[r][i] ^= c[r][vec_i] * data[i]. */
int rsgpu_ec_encode_data_update(rsgpu_ctx *ctx, int len, int k, int rows, int vec_i,
                                const unsigned char *gftbls, unsigned char *data,
                                unsigned char **coding);

/* The single-output / single-source members of the same ABI, as
 * isa_arithmetic and ISA-L's own tests call them (HOST tables and pointer
 * arrays, DEVICE rows, as rsgpu_ec_encode_data):
 *   erasure_code.h:637 gf_vect_dot_prod (isa/ec_base.c:264-276
 *     gf_vect_dot_prod_base): dest[i] = XOR_j c[j] * src[j][i], the 32*vlen
 *     tables of ONE output row; any len >= 0 (ISA-L asks len >= 32).
 *   erasure_code.h:664 gf_vect_mad (isa/ec_base.c:278-288): dest[i] ^=
 *     c[vec_i] * src[i], tables of vec coefficients.
 *   gf_vect_mul.h:108 gf_vect_mul (isa/ec_base.c:323-329): dest[i] =
 *     c * src[i] with c = gftbl[1]; returns 0, or non-zero when len is not a
 *     multiple of 32 (the dispatched ISA-L function's contract), and then
 *     writes nothing.
 * Each writes [0, len) of dest only (see rsgpu_ec_encode_data). */
int rsgpu_gf_vect_dot_prod(rsgpu_ctx *ctx, int len, int vlen, const unsigned char *gftbls,
                           unsigned char **src, unsigned char *dest);
int rsgpu_gf_vect_mad(rsgpu_ctx *ctx, int len, int vec, int vec_i, const unsigned char *gftbls,
                      unsigned char *src, unsigned char *dest);
int rsgpu_gf_vect_mul(rsgpu_ctx *ctx, int len, const unsigned char *gftbl, void *src, void *dest);

/* rsgpu_ec_encode_data over `blocks` blocks in one call, each block with its
 * own rows and its own length: for every block b and byte i < d_len[b]
 *   d_coding[b * rows + r][i] = XOR_j c[r][j] * d_data[b * k + j][i]
 * with c the rows x k matrix of the HOST tables `gftbls`, read exactly as
 * rsgpu_ec_encode_data reads them (one matrix for the whole call: parity rows
 * to encode, or a decode matrix applied to the rows that survived).
 *
 * d_data [blocks][k], d_coding [blocks][rows] (row pointers) and d_len
 * [blocks] are DEVICE memory, which the caller builds and may keep across
 * calls; they are only read.  The rows of a block need not be near each other,
 * and a row may be a source of many blocks; an output row that overlaps any
 * source or output row of the same call is undefined, as in ISA-L.  d_status
 * is DEVICE memory of [blocks] ints, or NULL.  max_len is the host's upper
 * bound of every d_len[b]: it sizes the launches, so nothing is read back from
 * the device.
 *
 * A block gets status -2 when d_len[b] < 0 or d_len[b] > max_len, and under
 * RSGPU_BATCH_ALIGNED32 also when its length is not a multiple of 32 or one of
 * its k + rows pointers is not 16-byte aligned; such a block is not touched.
 * Every other block gets status 0.  A block with d_len[b] == 0 is status 0
 * whatever its pointers are: none of them is looked at, they may be null.
 * RSGPU_BATCH_ALIGNED32 is the caller's promise that no block needs the byte
 * kernel, which is then not launched.
 *
 * k <= RSGPU_MAX_SOURCES and rows <= 255 as rsgpu_ec_encode_data; null tables
 * with rows > 0, max_len < 0 and unknown flags are RSGPU_ERR_ARG.  rows == 0
 * (only the lengths are judged then, and the pointer tables may be null),
 * blocks == 0 or max_len == 0 enqueue at most the status fill.  More than
 * 65535 blocks run as consecutive slices.  The call is enqueued on the
 * context's stream and does not synchronise, but for the first use of a
 * matrix, whose program is built then (as under RSGPU_ENCODE_GENERATED; the
 * context's cache of 64 programs), and for a growth of the context's scratch.
 * Under RSGPU_ENCODE_THREADED, or without an executable device memory pool,
 * the byte kernel serves every block whole; the statuses are the same.
 *
 * The call writes bytes [0, d_len[b]) of each of the `rows` output rows of
 * every block of status 0, the first `blocks` ints of d_status when given, and
 * nothing else: no byte of a source row, of the three tables, or behind a
 * row's length.  Of a source row it reads bytes [0, d_len[b]) only. */
#define RSGPU_BATCH_ALIGNED32 1 /* flags: every row 16-byte aligned, every d_len[b] % 32 == 0 */
int rsgpu_ec_encode_data_batch(rsgpu_ctx *ctx, int k, int rows, const unsigned char *gftbls,
                               size_t blocks, const unsigned char *const *d_data,
                               unsigned char *const *d_coding, const int *d_len, int max_len,
                               int flags, int *d_status);

/* ---- device, batched blocks (the benchmark hot path) --------------------- */

/* isa_encoder::encode_all over `blocks` independent blocks (isa.cpp:69-79):
 * parity[b][p] = XOR_j a[k+p][j] * src[b][j] with a = gf_gen_rs_matrix(k+e, k)
 * when `coef` is NULL, else with the HOST e x k row-major matrix `coef`.
 * src: [blocks][k] rows, parity: [blocks][e] rows, both at `pitch`.
 *
 * Under every encode kernel the call writes bytes [0, len) of each parity row
 * and nothing else: bytes in [len, pitch) of any row are never written, nor
 * is any byte of d_src.  len <= RSGPU_MAX_LEN (RSGPU_ERR_ARG beyond it,
 * nothing written). */
int rsgpu_encode_blocks(rsgpu_ctx *ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                        const unsigned char *d_src, unsigned char *d_parity,
                        const unsigned char *coef);

/* Encode kernel of rsgpu_encode_blocks / rsgpu_ec_encode_data (per context;
 * every choice writes the same bytes):
 *   AUTO       COMPILED for the codes built in (gf_gen_rs_matrix (k, e) in
 *              {(16,4) (16,8) (64,32) (64,16) (5,4) (20,7)}, no `coef`),
 *              otherwise GENERATED (aligned rows, len % 32 == 0; (100,20),
 *              compiled too, runs GENERATED: its compiled waves own 5 rows),
 *              otherwise the v_perm kernel; (64, 32) calls of at least
 *              480000 (2 KB column tile, block) pairs run KARATSUBA
 *   COMPILED   k_rs_bs: the matrix compiled into the kernel (codes above
 *              and (100,20))
 *   GENERATED  code built on the host for the matrix, once, shared by every
 *              block: per (wave, source) only the composites its
 *              coefficients need (greedy cover); 2 waves x 16 / 12 / 10 rows
 *              for 16 < e <= 32, 4 waves for 32 < e <= 64, passes of <= 64
 *              rows above (k_rs_jitw, the decode's layout), else waves of 8
 *              rows (k_rs_jit); the context keeps the last 64 programs (at
 *              most 256 MB of executable device memory, least recently
 *              used out), so a caller cycling through matrices builds each
 *              once
 *   THREADED   k_rs_tc: 256 generated handlers, one dispatch per coefficient
 *   KARATSUBA  the (64, 32) gf_gen_rs_matrix code through a generated program
 *              split by one Karatsuba level: three waves per column tile,
 *              each one 16 x 32 product, combined once per tile (k_rs_kara;
 *              aligned rows, len % 32 == 0); where it does not apply the
 *              choice behaves as AUTO
 * A choice that does not apply falls back in that order. */
#define RSGPU_ENCODE_AUTO 0
#define RSGPU_ENCODE_COMPILED 1
#define RSGPU_ENCODE_GENERATED 2
#define RSGPU_ENCODE_THREADED 3
#define RSGPU_ENCODE_KARATSUBA 4
int rsgpu_set_encode_kernel(rsgpu_ctx *ctx, int kernel);

/* Device workspace needed by rsgpu_decode_blocks for this geometry (any
 * decode kernel choice). */
size_t rsgpu_decode_workspace_bytes(int k, int e, size_t blocks);

/* Decode kernel of rsgpu_decode_blocks (per context; every choice recovers
 * the same bytes):
 *   AUTO        GENERATED when a block has >= 16 column tiles of 2 KB
 *               (len > 30 KiB), or fewer whose generated code is at most
 *               2 KB per tile, and the call has >= 4096 (block, tile)
 *               pairs, else ONE_MATRIX (the default)
 *   ONE_MATRIX  closed-form e x k decode rows V_E^-1 [V_kept | I] (e <= 32),
 *               one threaded-code pass over the k - e survivors + e parity;
 *               rsgpu_decode_blocks runs a small call (< 2048 (block, 2 KB
 *               column) pairs, e <= 8, k <= 64) as ONE launch that builds the
 *               rows itself (the prepare/apply pair keeps two); under AUTO a
 *               small call of a code with a compiled single-chunk program
 *               ((16,4) (16,8) (5,4) (20,7)) instead runs ONE launch of
 *               syndromes through that program plus the e x e solve
 *   GENERAL     the reference's k x k survivor-matrix inversion on the
 *               device (isa.cpp:177-204), then the decode rows; any e
 *   GENERATED   the ONE_MATRIX rows baked into per-block straight-line code
 *               (written to executable device memory by the prepare step),
 *               one call per chunk of sources: 2 waves x 16 rows for
 *               24 < e <= 32 (k_rs_jit16), x 12 rows for 20 < e <= 24
 *               (k_rs_jit12), x 10 rows for 16 < e <= 20 (k_rs_jit10),
 *               4 waves of 10 / 12 / 16 rows for 32 < e <= 40 / 48 / 64
 *               (k_rs_jit{10,12,16}x4), passes of <= 64 rows for e > 64
 *               (closed-form rows for every e; AUTO takes it for e > 32
 *               when the code pays for itself -- enough column tiles per
 *               block, jit_pays -- and otherwise runs GENERAL), else waves
 *               of 8 rows (k_rs_jit, e <= 16)
 * A choice that does not apply to a geometry falls back to GENERAL (e > 32,
 * unaligned rows) or ONE_MATRIX. */
#define RSGPU_DECODE_AUTO 0
#define RSGPU_DECODE_ONE_MATRIX 1
/* Deprecated alias: 2 selected a fused syndrome + solve kernel (removed in
 * round 3, never faster).  It is still accepted and runs ONE_MATRIX, which
 * writes the same bytes. */
#define RSGPU_DECODE_FUSED 2
#define RSGPU_DECODE_GENERAL 3
#define RSGPU_DECODE_GENERATED 4
int rsgpu_set_decode_kernel(rsgpu_ctx *ctx, int kernel);

/* isa_decoder::decode_all over `blocks` blocks (isa.cpp:169-213): for block
 * b the `e` erased ORIGINAL indices d_err[b][0..e-1] (strictly ascending, as
 * the std::set iterates, isa.cpp:150-153) are rebuilt from the surviving
 * originals and all e parity rows.  On the device: survivor matrix ->
 * gf_invert_matrix -> decode rows -> dot product into out[b][i] (symbol
 * d_err[b][i]).  The erased rows of d_src are never read.  d_status[b] = 0;
 * -1 for a singular matrix ("BAD MATRIX", isa.cpp:185-190); -2 for a
 * malformed erasure list (not strictly ascending, or an index >= k).  A
 * block with a non-zero status is skipped; its output is unspecified.
 * d_workspace holds rsgpu_decode_workspace_bytes() bytes.  Batches of more
 * than 65535 blocks run as consecutive slices (as do rsgpu_encode_blocks,
 * rsgpu_decode_general and rsgpu_verify_blocks).
 *
 * What the call writes, under every decode kernel: bytes [0, len) of each of
 * the blocks x e rows of d_out, the first rsgpu_decode_workspace_bytes() bytes
 * of d_workspace and the first `blocks` ints of d_status.  Bytes in [len,
 * pitch) of any row are never written, nor is any byte of d_src, d_parity or
 * d_err, any byte of d_workspace beyond rsgpu_decode_workspace_bytes(), or any
 * int of d_status beyond `blocks`.  A block with a non-zero status has
 * unspecified bytes only in [0, len) of its own output rows.
 * len <= RSGPU_MAX_LEN (RSGPU_ERR_ARG beyond it, nothing written). */
int rsgpu_decode_blocks(rsgpu_ctx *ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                        const unsigned char *d_src, const unsigned char *d_parity,
                        const unsigned char *d_err, unsigned char *d_out, void *d_workspace,
                        int *d_status);

/* The two halves of rsgpu_decode_blocks, for callers that time or reuse them:
 * prepare = survivor matrix + gf_invert_matrix + decode tables + row pointers
 * (isa.cpp:177-207) into d_workspace and d_status; apply = the dot product
 * (isa.cpp:208-209) for blocks whose status is 0.  decode_blocks ==
 * prepare followed by apply on the same stream.  At most 65535 blocks per
 * call (RSGPU_ERR_ARG beyond).  apply must be given the geometry, block
 * count, buffers and workspace of the prepare before it, with no
 * rsgpu_set_decode_kernel in between: both derive the decode kernel (and so
 * the workspace layout) from them.  The generated-code decode keeps the code
 * of the context's LAST prepare: an apply whose (k, e, blocks, workspace)
 * differ from it, or that follows another decode call on the context (which
 * rewrites or regrows the code), returns RSGPU_ERR_ARG and launches nothing.
 *
 * Together the two write what rsgpu_decode_blocks writes, and never what it
 * never writes: the prepare only the first rsgpu_decode_workspace_bytes()
 * bytes of d_workspace and the first `blocks` ints of d_status (no byte of
 * d_out), the apply only bytes [0, len) of the rows of d_out.
 * len <= RSGPU_MAX_LEN (RSGPU_ERR_ARG beyond it, nothing written). */
int rsgpu_decode_prepare(rsgpu_ctx *ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                         const unsigned char *d_src, const unsigned char *d_parity,
                         const unsigned char *d_err, unsigned char *d_out, void *d_workspace,
                         int *d_status);
int rsgpu_decode_apply(rsgpu_ctx *ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                       const unsigned char *d_src, const unsigned char *d_parity,
                       unsigned char *d_out, void *d_workspace, const int *d_status);

/* General erasure decode: ISA-L's gf_gen_decode_matrix + recovery
 * (isa-l_open_src_2.13/erasure_code/erasure_code_base_test.c:133-213, :292-
 * 308) for any m x k encode matrix and erasures among data AND parity rows.
 *   encode_matrix  HOST m x k row-major (identity on top, as gf_gen_rs_matrix
 *                  / gf_gen_cauchy1_matrix make it), or NULL for
 *                  gf_gen_rs_matrix(m, k)
 *   d_src [blocks][k] rows, d_parity [blocks][m-k] rows (pitch `pitch`)
 *   d_err [blocks][nerrs] erased row indices in [0, m), strictly ascending
 *   d_out [blocks][nerrs] recovered rows, in d_err order
 * Survivors are the first k rows not erased, ascending; when their matrix is
 * singular the reference's retry (replace the last survivor by a later row,
 * :163-184) runs, and only when that fails the block gets status -1 ("BAD
 * MATRIX").  Status -2: malformed list (not ascending, index >= m, or more
 * than m - k erasures).  Erased rows are never read.
 *
 * The call writes bytes [0, len) of each of the blocks x nerrs rows of d_out,
 * the first rsgpu_decode_general_workspace_bytes() bytes of d_workspace and
 * the first `blocks` ints of d_status.  Bytes in [len, pitch) of any row are
 * never written, nor is any byte of d_src, d_parity or d_err, any byte of
 * d_workspace beyond that size, or any int of d_status beyond `blocks`.  A
 * block with a non-zero status has unspecified bytes only in [0, len) of its
 * own output rows.
 * len <= RSGPU_MAX_LEN (RSGPU_ERR_ARG beyond it, nothing written). */
size_t rsgpu_decode_general_workspace_bytes(int k, int m, int nerrs, size_t blocks);
int rsgpu_decode_general(rsgpu_ctx *ctx, int k, int m, size_t len, size_t pitch, size_t blocks,
                         const unsigned char *encode_matrix, const unsigned char *d_src,
                         const unsigned char *d_parity, const unsigned char *d_err, int nerrs,
                         unsigned char *d_out, void *d_workspace, int *d_status);

/* isa_decoder::verify_data (isa.cpp:215-229) on the device: adds to
 * d_mismatch[b] the number of bytes where out[b][i] != src[b][d_err[b][i]].
 * len <= RSGPU_MAX_LEN (RSGPU_ERR_ARG beyond it, nothing written). */
int rsgpu_verify_blocks(rsgpu_ctx *ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                        const unsigned char *d_src, const unsigned char *d_out,
                        const unsigned char *d_err, unsigned long long *d_mismatch);

/* ---- parity scrub: are the k + e rows of a block still consistent? ------- */

/* Per byte column i of a block, with the e x k parity matrix c (`coef`, or
 * rows k..k+e-1 of gf_gen_rs_matrix(k+e, k) when NULL), the syndromes are
 *   s_p = parity[p][i] ^ XOR_j c[p][j] * src[j][i],   p < e,
 * and the column is BAD when any s_p != 0.  A bad column is explained by
 *   source row r < k    when some x != 0 has s_p = c[p][r] * x for every p,
 *   parity row k + p0   when s_p != 0 exactly for p = p0.
 * A matrix is LOCATABLE when e >= 2, its rows 0 and 1 have no zero entry and
 * the k ratios c[1][j] / c[0][j] are pairwise distinct: then at most one row
 * explains a column (the gf_gen_rs_matrix code, ratios 2^j, and
 * gf_gen_cauchy1_matrix both are).
 *
 * The report of a block (overwritten by every call, never accumulated):
 *   CLEAN     no bad column
 *   ONE_ROW   (RSGPU_SCRUB_LOCATE only) every bad column is explained by the
 *             same row, `row` in [0, k + e)
 *   DAMAGED   anything else: a column no row explains, two columns that point
 *             at different rows, or any bad column without RSGPU_SCRUB_LOCATE
 * ONE_ROW names the most likely explanation, not a proof: a code of distance
 * e + 1 tells damage in one row of a column from damage in up to e - 1 rows,
 * so with e = 2 two damaged rows in one column can look like a third. */
#define RSGPU_SCRUB_CLEAN 0
#define RSGPU_SCRUB_ONE_ROW 1
#define RSGPU_SCRUB_DAMAGED 2
typedef struct rsgpu_scrub_report {
    unsigned long long bad_columns; /* number of bad byte columns in [0, len) */
    int status;                     /* RSGPU_SCRUB_CLEAN / _ONE_ROW / _DAMAGED */
    int row;                        /* ONE_ROW: the row in [0, k+e); otherwise -1 */
} rsgpu_scrub_report;

#define RSGPU_SCRUB_LOCATE 1 /* flags: name the one damaged row where there is one */

/* Scrubs `blocks` blocks (layout as rsgpu_encode_blocks; d_src and d_parity
 * are only read) into d_report [blocks] (DEVICE memory, 8-byte aligned).
 * Enqueued on the context's stream, no synchronisation.  Any geometry
 * rsgpu_encode_blocks accepts; e == 0 or len == 0 reports every block CLEAN.
 * RSGPU_SCRUB_LOCATE with a matrix that is not locatable (e < 2 included)
 * returns RSGPU_ERR_UNSUPPORTED and enqueues nothing.
 * len <= RSGPU_MAX_LEN (RSGPU_ERR_ARG beyond it, nothing written). */
int rsgpu_scrub_blocks(rsgpu_ctx *ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                       const unsigned char *d_src, const unsigned char *d_parity,
                       const unsigned char *coef, int flags, rsgpu_scrub_report *d_report);

/* Host only: 1 when the e x k matrix `coef` (NULL: the gf_gen_rs_matrix
 * code) is locatable by the rule above, else 0. */
int rsgpu_scrub_locatable(int k, int e, const unsigned char *coef);

/* Scrub kernel of rsgpu_scrub_blocks (per context; every choice writes the
 * same reports):
 *   AUTO      FUSED wherever it applies, otherwise TWO_PASS
 *   FUSED     k_rs_bs_scrub: the compiled encode programs ((16,4) (16,8)
 *             (64,32) (64,16) (100,20) (5,4) (20,7), no `coef`, 16-byte
 *             aligned rows, len % 32 == 0) with the stored parity read and
 *             compared in registers; a clean tile writes nothing
 *   TWO_PASS  the parity of a slice of blocks computed into context-owned
 *             scratch (at most 128 MiB, or one block's parity when that is
 *             larger) by the encode dispatch, then k_scrub_compare; any
 *             geometry
 *   GENERATED the generated encode's shared program of the call's matrix
 *             (built once per matrix and context, the one a GENERATED encode of
 *             the same matrix runs) with FUSED's epilogue for a matrix known
 *             at run time (k_rs_jit_scrub): any matrix, with or without
 *             `coef`, for 1 <= e <= 64, 16-byte aligned rows (pitch % 16 == 0),
 *             len % 32 == 0 and len < 4 GiB, on a device with an executable
 *             memory pool; no parity scratch, a clean tile writes nothing.
 *             Opt-in: AUTO never takes it.  rsgpu_repair_blocks does not use
 *             it: under GENERATED the repair runs its TWO_PASS form; its own
 *             generated form is rsgpu_set_repair_kernel's GENERATED (below,
 *             at rsgpu_repair_blocks).  rsgpu_scrub_degraded_blocks, and the
 *             check of rsgpu_rebuild_blocks with it, does under
 *             rsgpu_set_degraded_kernel's FUSED (below) and not otherwise: the
 *             two settings together select the generated degraded scrub for
 *             the matrices that are not compiled in.  rsgpu_locate_blocks does, under
 *             rsgpu_set_locate_kernel's FUSED (below): the two settings
 *             together select the generated locate.  rsgpu_correct_blocks
 *             does likewise, under rsgpu_set_correct_kernel's FUSED (below),
 *             for the matrices that are not compiled in.
 *             Measured on an MI355X, 1 MB rows, 1.5 GB of rows per call, clean
 *             data, kernel times, medians of 24 runs: (10,4) 0.37 ms against
 *             0.49 ms TWO_PASS (gf_gen_rs_matrix and Cauchy alike), (6,3) 0.40
 *             / 0.54, (12,4) 0.35 / 0.45, (17,3) 0.32 / 0.39, (20,7) 0.37 /
 *             0.47, (64,32) 0.40 / 0.56: 0.70 - 0.82 of TWO_PASS, no shape
 *             loses to it.  It is not the generated encode's time, as FUSED is
 *             the compiled encode's: 1.05 ((64,32)) to 1.27 ((6,3)) of the
 *             GENERATED encode of the same rows, and 1.18 ((20,7)) and 1.34
 *             ((64,32)) of FUSED, which stays the faster choice for the
 *             compiled codes (profiles/scrub_generated/).
 * A choice that does not apply falls back to TWO_PASS. */
#define RSGPU_SCRUB_AUTO 0
#define RSGPU_SCRUB_FUSED 1
#define RSGPU_SCRUB_TWO_PASS 2
#define RSGPU_SCRUB_GENERATED 3
int rsgpu_set_scrub_kernel(rsgpu_ctx *ctx, int kernel);

/* ---- degraded scrub: a block with known-lost rows ------------------------ */

/* A block may have rows that are KNOWN to be lost (a failed device), and one
 * of its surviving rows may be silently bad as well.  The decodes trust every
 * survivor, and the scrub above needs all k + e rows: run after a rebuild it
 * sees the error only in the parity rows the decoder did not use and names a
 * healthy parity row.  This call answers, BEFORE anything is rebuilt, whether
 * the survivors are consistent, and with >= 2 spare parity rows which one
 * surviving row is not; the caller adds that row to the erasure list and
 * decodes with the calls above, or lets rsgpu_rebuild_blocks below do both on
 * the device.  Nothing is decoded and no row is written.
 *
 * Per byte column of a block with lost set L (n rows, n <= e):
 *   consistent  some choice of bytes for the rows in L makes all e syndromes
 *               (the scrub's s_p above) zero; BAD otherwise
 *   explains    a surviving row r explains a bad column when XORing some
 *               x != 0 into row r's byte makes the column consistent
 * Both are properties of the surviving bytes alone: the bytes stored in the
 * lost rows influence no field of any report.  The call may nevertheless READ
 * the lost source rows (they are part of the layout; its first pass is the
 * ordinary encode of all k rows); lost parity rows are never read.
 *
 *   d_lost  DEVICE [blocks][u] bytes, 1 <= u <= 8: block b's list of lost
 *           row indices in [0, k + e), strictly ascending (k + p is parity
 *           row p), then RSGPU_LOST_NONE to the end; n, the number of listed
 *           rows, may differ from block to block
 *   flags   0 or RSGPU_SCRUB_LOCATE
 *
 * The report (rsgpu_scrub_report, overwritten by every call): bad_columns is
 * the number of bad columns, row is -1 except for ONE_ROW, and the status is
 * the first that applies of
 *   BAD_LIST    not strictly ascending, an index >= k + e, a row after a
 *               NONE, or n > e; bad_columns 0; the compare reads nothing of
 *               the block beyond the list (the encode pass reads its source
 *               rows with the rest of the batch; they influence nothing)
 *   UNCHECKED   n == e: no spare row, nothing can be checked
 *   BAD_MATRIX  with D the lost data rows, no |D| surviving parity rows p
 *               have c[p][D] invertible: the survivors do not determine D
 *   CLEAN       no bad column
 *   ONE_ROW     (RSGPU_SCRUB_LOCATE only) every bad column is explained by
 *               EXACTLY one surviving row, the same in all of them: `row`
 *   DAMAGED     anything else, a column that no row or more than one row
 *               explains included.  With a spare of e - n == 1 no column is
 *               explained by exactly one row: such a block is CLEAN or DAMAGED
 * No matrix is refused as "not locatable": ambiguity is decided per column.
 * With every list all-NONE the reports equal rsgpu_scrub_blocks' byte for
 * byte for the gf_gen_rs_matrix and gf_gen_cauchy1_matrix codes (at most one
 * row explains a column there).  As the scrub's, ONE_ROW names the most
 * likely explanation, not a proof: e - n - 1 or more damaged survivors in one
 * column can look like another single row.
 *
 * Layout, `coef` and accepted geometries as rsgpu_scrub_blocks (any len, any
 * pitch >= len, any alignment, custom e x k matrix or NULL); d_report
 * [blocks] is DEVICE memory, 8-byte aligned.  Enqueued on the context's
 * stream, no synchronisation; more than 65535 blocks run as consecutive
 * slices.  e == 0 or len == 0: every block with a well-formed list is CLEAN,
 * a malformed list is still BAD_LIST.  Null pointers, a misaligned report, u
 * outside [1, 8] or unknown flag bits: RSGPU_ERR_ARG, nothing is enqueued and
 * the report is untouched.
 *
 * Cost: the encode of the k source rows into context-owned scratch (slices
 * of at most 128 MiB of parity, as the TWO_PASS scrub), then
 * k_degraded_compare, which reads the stored and the recomputed row of every
 * surviving parity row once: 2 (e - |P|) rows per block, P the lost parity
 * rows.  Measured at (64, 32), 1 MB rows, 1024 blocks on one MI355X
 * (profiles/degraded): one lost row per block 36.4 ms, what
 * the TWO_PASS scrub of complete blocks takes (36.2 ms; FUSED 22.3 ms, the
 * encode alone 22.0 ms); 4 lost rows 38.8 ms, 8 lost rows 41.5 ms.  The
 * compare is memory-bound for up to 2 lost data rows per block and bound by
 * its arithmetic at 8 (0.79 of the device-to-device copy rate).  A form fused
 * into the compiled encode is rsgpu_set_degraded_kernel's FUSED, below.  Not
 * built: host-resident blocks. */
#define RSGPU_LOST_NONE 255         /* list padding */
#define RSGPU_SCRUB_UNCHECKED 3     /* n == e: no spare row, nothing can be checked */
#define RSGPU_SCRUB_BAD_MATRIX (-1) /* the lost data rows are not determined by the surviving parity */
#define RSGPU_SCRUB_BAD_LIST (-2)   /* malformed list */
/* len <= RSGPU_MAX_LEN (RSGPU_ERR_ARG beyond it, nothing written). */
int rsgpu_scrub_degraded_blocks(rsgpu_ctx *ctx, int k, int e, size_t len, size_t pitch,
                                size_t blocks, const unsigned char *d_src,
                                const unsigned char *d_parity, const unsigned char *coef,
                                int u, const unsigned char *d_lost, int flags,
                                rsgpu_scrub_report *d_report);

/* Kernel of rsgpu_scrub_degraded_blocks, and with it of the check that
 * rsgpu_rebuild_blocks runs under RSGPU_REBUILD_CHECK (per context; every
 * choice writes the same reports):
 *   AUTO      TWO_PASS
 *   TWO_PASS  the encode into scratch, then k_degraded_compare (the cost
 *             above); any geometry
 *   FUSED     k_rs_bs_degraded, between k_degraded_prepare and
 *             k_degraded_finalise in place of the encode and the compare: the
 *             compiled encode programs with the stored parity read and the
 *             syndromes reduced and compared in registers, as FUSED of
 *             rsgpu_set_scrub_kernel and where it applies -- (16,4) (16,8)
 *             (64,32) (64,16) (100,20) (5,4) (20,7), no `coef`, pitch % 16 == 0,
 *             16-byte aligned d_src and d_parity, len % 32 == 0, len < 4 GiB.
 *             No encode is launched and the parity scratch is neither touched
 *             nor grown; a workgroup whose block the prepare has reported loads
 *             nothing, a lost parity row is never read, a clean tile writes
 *             nothing.  Where that form does not apply and the context's scrub
 *             kernel is RSGPU_SCRUB_GENERATED (rsgpu_set_scrub_kernel), the
 *             generated form, k_rs_jit_degraded, in the same place: the
 *             generated encode's shared program of the call's matrix (the one
 *             a GENERATED encode or scrub of it runs, built once per matrix
 *             and context) with the same reduction for a matrix known at run
 *             time -- any matrix, with or without `coef`, for e <= 64,
 *             pitch % 16 == 0, 16-byte aligned d_src and d_parity,
 *             len % 32 == 0 and len < 4 GiB, on a device with an executable
 *             memory pool; the compiled form has precedence where both apply.
 *             The same holds of it: no encode, no parity scratch, a reported
 *             block's workgroups load nothing, a lost parity row is never
 *             read, a clean workgroup writes nothing.  Every layout of the
 *             generated scrub has this form (none falls back for registers).
 *             Any other call runs TWO_PASS, silently.  Opt-in: AUTO does not
 *             take either form yet.
 * Of rsgpu_set_scrub_kernel's choices only GENERATED has an influence on these
 * calls, and only under FUSED, as above; AUTO and TWO_PASS here ignore it.
 * The generated form is not measured yet (tools/degraded_measure.py
 * --generated, profiles/degraded_generated): expected from the generated
 * locate and repair is the generated scrub's time on clean blocks and, at
 * small e, a loss to TWO_PASS on damaged ones, whose cold path is small code
 * and not fast code.
 * Measured at (64, 32), 1 MB rows, 1024 blocks on one MI355X, both choices in
 * mirrored pairs in one process, medians of 24 runs, FUSED / TWO_PASS and the
 * spread of the pairs' ratio (profiles/degraded_fused), clean
 * survivors: all-NONE lists 21.9 / 36.0 ms (0.60 - 0.69; the FUSED
 * rsgpu_scrub_blocks of the same blocks 22.5 ms); one lost data row 23.9 / 36.3
 * (0.65 - 0.67); one lost parity row 21.8 / 35.5 (0.60 - 0.63); 4 lost rows
 * 27.3 / 37.3 (0.72 - 0.74); 8 lost data rows 35.3 / 42.9 (0.81 - 0.83); lists
 * of 0 to 8 rows mixed 27.4 / 37.5 (0.72 - 0.74).  One surviving row bad in 1 %
 * of the columns, one lost data row: 141.6 / 174.8 ms (0.81), the cold path on
 * both sides.  The checked rebuild at n = 1 / 4 / 7: 35.5 / 42.2 / 51.3 ms
 * against 47.8 / 52.1 / 59.7.  A lost parity row costs nothing, a lost data row
 * 1.6 - 2.0 ms (one more pivot in the reduction on planes); FUSED did not lose
 * to TWO_PASS at any number of lost rows a list can hold. */
#define RSGPU_DEGRADED_AUTO 0
#define RSGPU_DEGRADED_TWO_PASS 1
#define RSGPU_DEGRADED_FUSED 2
int rsgpu_set_degraded_kernel(rsgpu_ctx *ctx, int kernel);

/* ---- rebuild in place of known-lost rows, optionally checked -------------- */

/* The step after the degraded scrub: the rows a block's list names are
 * rebuilt where they belong, lost parity rows included, batched and on the
 * stream.  Lists may hold a different number of rows in every block, which
 * rsgpu_decode_general (one nerrs for the batch, a separate d_out) does not
 * take.  With RSGPU_REBUILD_CHECK the degraded scrub runs first and its
 * verdict decides per block, on the device and with no host decision in
 * between, what is written: a silently bad survivor is rebuilt with the lost
 * rows instead of being sealed into them.
 *
 * Layout, `coef` and d_lost exactly as rsgpu_scrub_degraded_blocks: [blocks][u]
 * bytes, rows in [0, k + e) strictly ascending, then RSGPU_LOST_NONE; n may
 * differ from block to block.  Any len, any pitch >= len, any alignment.
 * Without RSGPU_REBUILD_CHECK u is in [1, max(8, min(e, RSGPU_REBUILD_MAX_LOST))]:
 * everything up to 8, and beyond 8 a list as long as the code has parity rows,
 * up to 32; with RSGPU_REBUILD_CHECK u is in [1, 7]: the located row may join
 * the list, and the degraded scrub holds at most 8 rows per lane.  d_report
 * [blocks] is the 16-byte rsgpu_scrub_report, DEVICE memory, 8-byte aligned,
 * overwritten by every call.
 *
 * Rebuilt, for a block with list L and D the lost data rows of L: the pivot
 * rows Q are the surviving parity rows, walked in ascending order, that each
 * raise the rank of c[Q][D]; the lost data bytes are the unique solution that
 * zeroes the syndromes of the rows in Q; every lost parity row is the encode
 * of the completed data.  With consistent survivors the result is the
 * original block and does not depend on Q.  With inconsistent survivors it is
 * defined by the greedy Q, for the gf_gen_rs_matrix and gf_gen_cauchy1_matrix
 * codes the first |D| surviving parity rows, and then equals byte for byte
 * what rsgpu_decode_general (ISA-L's gf_gen_decode_matrix path) recovers for
 * the same list.
 *
 * Status per block, the first that applies:
 *   BAD_LIST    a malformed list or n > e, as in the degraded scrub; nothing
 *               of the block is read or written by the rebuild
 *   BAD_MATRIX  the surviving parity rows do not determine D, judged on the
 *               list as it will be rebuilt and also when n == e (where the
 *               degraded scrub says UNCHECKED without looking at the matrix);
 *               nothing is written
 *   without RSGPU_REBUILD_CHECK: CLEAN, bad_columns 0, row -1, every listed
 *               row rebuilt (n == 0 writes nothing)
 *   with RSGPU_REBUILD_CHECK: the report is what rsgpu_scrub_degraded_blocks
 *               with RSGPU_SCRUB_LOCATE reports for the block as it was before
 *               the call, and
 *     CLEAN      the listed rows are rebuilt
 *     UNCHECKED  (n == e) the listed rows are rebuilt on trust; the status
 *                tells the caller so
 *     ONE_ROW    `row` joins the list and L + {row} is rebuilt: all len bytes
 *                of that row are rewritten, in its consistent columns with the
 *                value they had
 *     DAMAGED    nothing is written
 * A located row can always join the list: a row that explains a column has a
 * non-zero reduced column, so the surviving parity rows still determine the
 * extended D.  As the scrub's, ONE_ROW is the most likely explanation, not a
 * proof: with e - n - 1 or more damaged survivors in one column the checked
 * rebuild can write a consistent but wrong block.
 *
 * e == 0 or len == 0: every well-formed list is CLEAN and nothing is written;
 * a malformed list is still BAD_LIST.  Null pointers, a misaligned report, u
 * out of range for the mode or unknown flag bits: RSGPU_ERR_ARG, nothing is
 * enqueued and the report is untouched.  Enqueued on the context's stream, no
 * synchronisation; more than 65535 blocks run as consecutive slices.  Listed
 * rows are never read without RSGPU_REBUILD_CHECK; with it only the scrub's
 * encode pass reads the lost source rows, and they influence nothing.  Never
 * written: surviving rows (other than a located row), bytes in [len, pitch),
 * and the lists.
 *
 * Cost: k_rebuild_prepare (one wave per block: the pivots, the inverse and
 * the block's k x 8 matrix of factors), then k_rebuild_blocks, ONE walk over k
 * surviving rows per block -- the surviving data rows and the |D| pivot parity
 * rows -- that writes the listed rows: (k + n) rows of traffic per block, no
 * encode into scratch.  RSGPU_REBUILD_CHECK adds the degraded scrub in front
 * (its cost above).  The vector path needs pitch % 16 == 0 and 16-byte
 * aligned d_src and d_parity; other layouts run a byte kernel.  Measured at
 * (64, 32), 1 MB rows, 1024 blocks on one MI355X (profiles/rebuild, DESIGN.md
 * 3.8; the device-to-device copy of the same bytes ran at 5.04 TB/s): one lost
 * row per block 11.8 ms, two 12.8 ms, four 14.5 ms -- the bytes at the copy's
 * rate within 5 % -- and eight 22.8 ms, 1.56 of its bytes: with 8 outputs per
 * lane the kernel is bound by its arithmetic (172 instructions per 16-byte
 * column and source).  rsgpu_decode_general with the same uniform lists took
 * 11.9 / 12.2 / 13.2 / 15.5 ms: equal at one row, 5 % and 9 % faster at two
 * and four, 1.48 x faster at eight.  Checked, with clean survivors: 46.8 ms
 * (n = 1), 51.2 ms (n = 4), 58.5 ms (n = 7), the degraded scrub alone being
 * 34.9 / 36.5 / 38.0 ms.
 *
 * Lists of more than 8 rows, and rsgpu_set_rebuild_kernel below: LANES runs
 * k_rebuild_blocks in passes of at most 8 outputs, one more walk over the k
 * sources each; THREADED runs k_rs_tc, the bit-sliced threaded code of the
 * encode and decode, once for up to 32 rows, with a row count per block and
 * the rows written in place, after k_rebuild_wide_prepare (one wave per block,
 * the elimination spread over the wave) has written its row pointers and
 * handler addresses, 16 KB per block at k = 64, into a context-owned buffer of
 * at most 64 MiB per group of blocks.  Measured in one process at the same
 * shape with the same n rows lost in every block (profiles/rebuild_wide; the
 * copy ran at 4.85 TB/s), n = 8 / 16 / 32: THREADED 21.1 / 22.0 / 28.7 ms, LANES
 * 23.1 / 45.8 / 92.3 ms, THREADED the faster one in every mirrored pair;
 * rsgpu_decode_general with the same lists 16.3 / 18.2 / 23.6 ms; lists of 0 to
 * 32 rows mixed in one call: THREADED 22.5 ms, LANES 55.0 ms; the wide prepare
 * 0.1 / 0.2 / 0.6 ms of the call.  AUTO therefore takes THREADED above 8 rows
 * and, for now, leaves u + check <= 8 on LANES.  A caller whose blocks ALL
 * lose the same number of rows, whose survivors are trusted and who does not
 * need the rows in place is served 1.2 - 1.3 x faster by rsgpu_decode_general;
 * this call is for lists that differ from block to block, for rows that
 * should come back in place, and for the check.  Not built: host-resident
 * blocks, a generated-code form, the check with more than 7 listed rows, and
 * lists of more than 32 rows.  (Several damaged rows per block are located by
 * rsgpu_locate_blocks below, whose lists this call takes as they are.) */
#define RSGPU_REBUILD_CHECK 1 /* flags: scrub the survivors first, let the verdict decide */
#define RSGPU_REBUILD_MAX_LOST 32 /* the longest list without RSGPU_REBUILD_CHECK (and at most e) */
/* len <= RSGPU_MAX_LEN (RSGPU_ERR_ARG beyond it, nothing written). */
int rsgpu_rebuild_blocks(rsgpu_ctx *ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                         unsigned char *d_src, unsigned char *d_parity,
                         const unsigned char *coef, int u, const unsigned char *d_lost,
                         int flags, rsgpu_scrub_report *d_report);

/* Kernel of rsgpu_rebuild_blocks (per context; every choice writes the same
 * bytes and reports):
 *   AUTO      LANES whenever u + check <= 8; for longer lists THREADED where
 *             it applies, otherwise LANES
 *   LANES     k_rebuild_blocks: a lane holds up to 8 outputs of its column;
 *             lists longer than 8 run in passes of at most 8 outputs, each one
 *             more walk over the k sources (the passes are independent: no row
 *             is both read and written); any layout
 *   THREADED  k_rs_tc, the bit-sliced threaded code of the encode and decode,
 *             with a row count per block and the rows written in place; needs
 *             pitch % 16 == 0, 16-byte aligned d_src and d_parity and
 *             32 <= len < 4 GiB; covers the columns [0, len - len % 32), the
 *             last len % 32 bytes of every row go through LANES' byte form
 * A choice that does not apply falls back to LANES. */
#define RSGPU_REBUILD_AUTO 0
#define RSGPU_REBUILD_LANES 1
#define RSGPU_REBUILD_THREADED 2
int rsgpu_set_rebuild_kernel(rsgpu_ctx *ctx, int kernel);

/* ---- several damaged rows per block, located -------------------------------- */

/* The scrub names at most one row per block; a block damaged in two or more
 * rows (a torn write across two devices, two bad sectors in one stripe) ends
 * there as DAMAGED.  This call names up to min(u, e - 1) rows, in the list
 * format rsgpu_rebuild_blocks takes, from all the block's columns together:
 *
 *   s     the block's syndromes as the scrub defines them (stored ^ recomputed
 *         parity), one column of e bytes per byte column of the block
 *   h_r   what a unit change of row r adds to the syndromes: column r of the
 *         matrix for a data row, the unit vector of p for parity row k + p
 *   W     the span of the block's non-zero syndrome columns, d = dim W
 *   R     { r in [0, k + e) : h_r in W }
 *
 * Status per block:
 *   CLEAN             no bad column; the list is all RSGPU_LOST_NONE
 *   ONE_ROW           d <= u, |R| = d, rank(h_R) = d, and d == 1: `row` is the
 *                     row, the list holds it
 *   RSGPU_SCRUB_ROWS  the same with d >= 2: the list holds R, `row` its lowest
 *   DAMAGED           anything else (d > u, |R| != d, or h_R dependent): `row`
 *                     is -1 and the list all RSGPU_LOST_NONE
 * bad_columns is the number of non-zero syndrome columns, as in the scrub.  No
 * matrix is refused.  For a locatable matrix (rsgpu_scrub_locatable)
 * rsgpu_scrub_blocks with RSGPU_SCRUB_LOCATE reports CLEAN or ONE_ROW on
 * exactly the blocks where this call does, with all three fields equal.
 *
 * Two properties:
 *   1. rank(h_R) = |R| is exactly the condition under which
 *      rsgpu_rebuild_blocks does not answer BAD_MATRIX for the list (the lost
 *      data rows are determined by the surviving parity rows when the columns
 *      of the listed rows are independent).  Every located list can go
 *      straight into the rebuild; a DAMAGED block has an all-NONE list, which
 *      the rebuild leaves untouched.
 *   2. When the damage lies in fewer than e rows R' of a matrix whose every e
 *      columns of [C | I] are independent (MDS: gf_gen_cauchy1_matrix always),
 *      the verdict is R' exactly or DAMAGED, never another set: W lies in
 *      span(h_R'), so a row outside R' with h_r in W would make |R'| + 1 <= e
 *      columns dependent, hence R is a subset of R'; and |R| = d = rank(h_R)
 *      makes span(h_R) = W, which holds every syndrome column, so rows of R'
 *      outside R carry no damage.  DAMAGED arises when the damage patterns do
 *      not span all of span(h_R') (two rows hit only in the same single
 *      column).  Without the MDS property a dependent extra row makes
 *      |R| > d, and the block is DAMAGED.
 * As the scrub's ONE_ROW, a verdict is the explanation with the fewest rows,
 * not a proof: damage in e or more rows can imitate it.
 *
 * Layout, `coef` and accepted geometries as rsgpu_scrub_blocks: any len, any
 * pitch >= len, any alignment; additionally 1 <= e <= 64 where there is work
 * (e > 64: RSGPU_ERR_UNSUPPORTED, nothing enqueued).  d_rows is DEVICE memory,
 * [blocks][u] bytes, 1 <= u <= RSGPU_LOCATE_MAX_ROWS, written in the d_lost
 * format of rsgpu_rebuild_blocks: rows ascending, then RSGPU_LOST_NONE.
 * d_report [blocks] is DEVICE memory, 8-byte aligned, overwritten by every
 * call.  Nothing of d_src or d_parity is written.  e == 0 or len == 0: every
 * block CLEAN.  e == 1: any bad column gives DAMAGED (W is everything, R every
 * row).  Null pointers, a misaligned report or u outside [1, 8]:
 * RSGPU_ERR_ARG, nothing enqueued, outputs untouched.  Enqueued on the
 * context's stream, no synchronisation; more than 65535 blocks run as
 * consecutive slices.
 *
 * Cost: the TWO_PASS scrub's -- the encode of a slice into the context's
 * scratch, then k_locate_span, whose lanes read stored and recomputed parity
 * once as k_scrub_compare's do -- plus, per bad byte column, one
 * wave-cooperative reduction against a basis of at most u vectors (lane p
 * holds syndrome p: one cross-lane read and one table multiply per lane and
 * basis vector), and k_locate_finish, one wave per block (at most (k + e) d
 * reduction steps).  Workgroups leave their bases in a context-owned candidate
 * area of at most 64 MiB per group of blocks.  The result is a function of the
 * block alone.  Measured at (64, 32), 1 MB rows, 1024 blocks on one MI355X
 * (profiles/locate; the device-to-device copy ran at 5.14 TB/s):
 * clean blocks 34.85 ms, the TWO_PASS scrub with RSGPU_SCRUB_LOCATE in the same
 * process 34.66 ms (ratio 0.968 - 1.017 over 24 mirrored pairs, inside the
 * pair's run-to-run spread); one row per block bad in 1 % of the columns 50.4
 * ms, two rows 56.1 ms: a bad 16-byte column stops its wave's other 63 and
 * costs about 1.5 ns over the device.  Blocks damaged in most of their columns
 * are the worst case, every column taking the cooperative path: two whole
 * rows bad per block 175.6 ms, 5 x the scrub.  The form fused into the
 * encode, compiled or generated, is rsgpu_set_locate_kernel's FUSED, below.  Not built:
 * e > 64; u > 8.  Blocks that end DAMAGED with at most two damaged rows in any
 * one byte column: rsgpu_correct_blocks, below. */
#define RSGPU_SCRUB_ROWS 4        /* the damage lies in exactly the 2..u listed rows */
#define RSGPU_LOCATE_MAX_ROWS 8
/* len <= RSGPU_MAX_LEN (RSGPU_ERR_ARG beyond it, nothing written). */
int rsgpu_locate_blocks(rsgpu_ctx *ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                        const unsigned char *d_src, const unsigned char *d_parity,
                        const unsigned char *coef, int u, unsigned char *d_rows,
                        rsgpu_scrub_report *d_report);

/* Kernel of rsgpu_locate_blocks (per context; every choice writes the same
 * reports and lists):
 *   AUTO      TWO_PASS
 *   TWO_PASS  the encode of a slice into the context's scratch, then
 *             k_locate_span, as described above; any geometry
 *   FUSED     fused into the encode program of the call's matrix.  Where the
 *             compiled form applies it runs, and takes precedence:
 *             k_rs_bs_locate, the FUSED scrub's kernel (the compiled encode
 *             programs with the stored parity read and compared in registers)
 *             whose cold path reduces a dirty tile's syndrome columns to a
 *             basis of at most u vectors, as k_locate_span does of its
 *             columns, and writes it to the next free slot of the block's
 *             candidate area; k_locate_finish then reads the slots that were
 *             claimed.  A clean tile writes nothing, there is no parity scratch
 *             and no encode launch: a clean block costs what the FUSED scrub
 *             costs.  Applies where the FUSED scrub does ((16,4) (16,8) (64,32)
 *             (64,16) (100,20) (5,4) (20,7), no `coef`, pitch % 16 == 0, 16-byte
 *             aligned d_src and d_parity, len % 32 == 0, len < 4 GiB) and one
 *             block's candidate area (ceil(len / 2048) slots of 528 bytes)
 *             fits 64 MiB.  Opt-in: AUTO does not take it yet.
 *             Measured at (64, 32), 1 MB rows, 1024 blocks on one MI355X, one
 *             process, medians of 24 runs (profiles/locate_fused, DESIGN.md
 *             3.9): clean blocks 21.00 ms, the FUSED scrub with
 *             RSGPU_SCRUB_LOCATE 21.57 ms (ratio 0.882 - 0.991 over 24 mirrored
 *             pairs: it met the scrub's time), TWO_PASS locate 35.31 ms; one
 *             row per block bad in 1 % of the columns 24.98 ms (TWO_PASS
 *             50.64), two rows 28.84 ms (56.45), two whole rows bad per block
 *             133.8 ms (175.9), still the worst case.
 *             Otherwise, when the context's scrub kernel is
 *             RSGPU_SCRUB_GENERATED (rsgpu_set_scrub_kernel: the family's
 *             opt-in to generated programs), the generated form:
 *             k_rs_jit_locate / k_rs_jitw_locate, the GENERATED scrub's kernels
 *             on the matrix's shared program (the one the GENERATED encode and
 *             scrub of that matrix run; built on first use, cached per
 *             context) with the same cold path, one claimed slot per dirty
 *             workgroup, and the same k_locate_finish.  Any matrix, with or
 *             without `coef`; 1 <= e <= 64, pitch % 16 == 0, 16-byte aligned
 *             d_src and d_parity, len % 32 == 0, len < 4 GiB, a device with an
 *             executable memory pool, and one block's candidate area within
 *             64 MiB.  No parity scratch, no encode launch, and the scrub's
 *             locate tables are not uploaded.
 *             Measured at 1 MB rows, about 1.5 GB of rows per call, one
 *             MI355X, one process, medians of 24 runs (profiles/locate_generated,
 *             DESIGN.md 3.9; generated locate / TWO_PASS locate, ms):
 *                                        (10,4) Cauchy  (6,3) Cauchy   (14,32)
 *               clean                    0.378 / 0.510  0.414 / 0.545  0.298 / 0.881
 *               one row bad in 1 %       1.59 / 1.19    1.96 / 1.25    1.51 / 1.56
 *               two rows bad in 1 % each 2.50 / 1.53    3.20 / 1.73    1.68 / 1.92
 *               two whole rows bad       47.0 / 8.3     72.2 / 13.6    6.19 / 5.91
 *             Clean blocks cost what the GENERATED scrub with
 *             RSGPU_SCRUB_LOCATE costs in the same process (0.374, 0.409, 0.295
 *             ms; ratio over 24 mirrored pairs 1.005, 1.009, 1.018, stdev 0.010
 *             - 0.019, inside the pair's run-to-run spread), 0.74, 0.76 and
 *             0.34 of TWO_PASS.  On damaged blocks the generated form LOSES to
 *             TWO_PASS wherever e is small: every dirty workgroup runs the
 *             GENERATED scrub's cold path, eight passes that load the stored
 *             rows again dword by dword, each load waited for, on one or two
 *             waves, before its columns are reduced.  Advice: take the
 *             combination for scrubbing, where nearly every block is clean;
 *             a caller who expects damage in most blocks of a call with e <=
 *             16 is served better by TWO_PASS (at (14,32) the two forms are
 *             within 13 % of each other on every damaged kind).
 * A choice that does not apply falls back to TWO_PASS, silently. */
#define RSGPU_LOCATE_AUTO 0
#define RSGPU_LOCATE_TWO_PASS 1
#define RSGPU_LOCATE_FUSED 2
int rsgpu_set_locate_kernel(rsgpu_ctx *ctx, int kernel);

/* ---- repair in place of what the scrub locates ---------------------------- */

/* "Bad", "explains" and "locatable" as for the scrub above.  A bad column is
 * CORRECTED only when exactly one row explains it:
 *   source row r < k    src[r][i]     ^= s_0 / c[0][r]
 *   parity row k + p0   parity[p0][i] ^= s_p0
 * after which all its syndromes are zero.  Modes:
 *   ONE_ROW   conservative: a block is written only when every bad column of
 *             it names the same row (the scrub's ONE_ROW).  Such a block
 *             reports REPAIRED, repaired_columns == bad_columns and `row`;
 *             any other bad block reports DAMAGED, repaired_columns == 0,
 *             row == -1, and none of its bytes is touched.
 *   COLUMNS   every bad column that exactly one row explains is corrected,
 *             whatever the block's other columns say; a column no row
 *             explains stays as it was.  REPAIRED when every bad column was
 *             corrected, DAMAGED when none, otherwise PARTIAL; `row` is the
 *             common row of the corrected columns, -1 when they lie in
 *             several rows or there is none.  Needs e >= 3: correcting one
 *             error per column while still detecting two takes distance
 *             e + 1 >= 2 * 1 + 2 = 4; with e = 2 (distance 3) a two-row
 *             error of a column can be exactly the syndrome pair of a third
 *             row, and only the agreement of the block's columns (ONE_ROW)
 *             speaks against it.
 * As the scrub's ONE_ROW, a correction follows the most likely explanation,
 * not a proof: e - 1 or more damaged rows in one column can look like another
 * single row and are then "corrected" into a consistent but wrong column.  In
 * particular ONE_ROW mode with e = 2 can still miscorrect two damaged rows of
 * one column.
 *
 * The report of a block is overwritten by every call, never accumulated.
 * Bytes in [len, pitch) are never written, nor is any byte of a row that is
 * not corrected, nor any byte of a column that is not bad. */
#define RSGPU_REPAIR_CLEAN 0    /* no bad column */
#define RSGPU_REPAIR_REPAIRED 1 /* every bad column corrected */
#define RSGPU_REPAIR_PARTIAL 2  /* COLUMNS only: some corrected, some left as they were */
#define RSGPU_REPAIR_DAMAGED 3  /* bad columns, nothing written to this block */
typedef struct rsgpu_repair_report {
    unsigned long long bad_columns;      /* before the repair */
    unsigned long long repaired_columns; /* columns whose byte was corrected */
    int status;
    int row; /* the one row every corrected column lay in; -1 when none or several */
} rsgpu_repair_report;                   /* 24 bytes */

#define RSGPU_REPAIR_ONE_ROW 0 /* mode: correct only blocks the scrub would call ONE_ROW */
#define RSGPU_REPAIR_COLUMNS 1 /* mode: correct every bad column exactly one row explains */

/* Scrubs `blocks` blocks as rsgpu_scrub_blocks with RSGPU_SCRUB_LOCATE does
 * (same layout, geometries, kernel choice by rsgpu_set_scrub_kernel and, on
 * top of it, rsgpu_set_repair_kernel below) and
 * corrects d_src / d_parity in place on the device; d_report [blocks] is
 * DEVICE memory, 8-byte aligned.  Enqueued on the context's stream, no
 * synchronisation and no host decision between locating and writing.
 * e == 0: every block CLEAN.  Otherwise a matrix that is not locatable
 * (e < 2 included), or COLUMNS with e < 3, returns RSGPU_ERR_UNSUPPORTED:
 * nothing is enqueued, the report is untouched.  len == 0: every block CLEAN.
 * Null rows, a null or misaligned report, an unknown mode: RSGPU_ERR_ARG,
 * likewise with nothing enqueued and the report untouched.  After any other
 * error (RSGPU_ERR_HIP, RSGPU_ERR_NOMEM: work may already be enqueued) the
 * report's contents are undefined and must not be read as verdicts; rows are
 * only ever written as described above, so a block is either as it was or
 * corrected.
 * len <= RSGPU_MAX_LEN (RSGPU_ERR_ARG beyond it, nothing written). */
int rsgpu_repair_blocks(rsgpu_ctx *ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                        unsigned char *d_src, unsigned char *d_parity,
                        const unsigned char *coef, int mode, rsgpu_repair_report *d_report);

/* Repair kernel of rsgpu_repair_blocks (per context; every choice writes the
 * same rows and the same reports):
 *   AUTO      what rsgpu_set_scrub_kernel decides: FUSED (k_rs_bs_repair)
 *             where it applies, otherwise TWO_PASS (the encode of all k rows
 *             into the parity scratch, then k_repair_compare)
 *   GENERATED the generated scrub (RSGPU_SCRUB_GENERATED above) with a
 *             correcting cold path (k_rs_jit_repair): the shared program of
 *             the call's matrix, the stored parity compared in registers, and
 *             the byte of a bad column corrected where the row is named, with
 *             all e syndromes of the column at hand.  ONE_ROW runs it twice
 *             around the finalise (locate, then the gated correction of the
 *             blocks that are to be written), COLUMNS once.  Applies under the
 *             generated scrub's conditions: any matrix, with or without
 *             `coef`, 1 <= e <= 64 (the repair itself needs a locatable matrix,
 *             and e >= 3 for COLUMNS), 16-byte aligned rows (pitch % 16 == 0),
 *             len % 32 == 0 and len < 4 GiB, on a device with an executable
 *             memory pool; no encode launch, and the parity scratch is neither
 *             touched nor grown.  Where it applies it comes before FUSED;
 *             where it does not, the call runs what AUTO runs, silently.
 *             Opt-in: neither the default nor AUTO takes it, and
 *             rsgpu_set_scrub_kernel(GENERATED) alone leaves the repair on its
 *             TWO_PASS form.
 *             Measured on an MI355X, 1 MB rows, 1.5 GB of rows per call, kernel
 *             times, medians of 24 runs (profiles/repair_generated/).
 *             Clean data: COLUMNS is the GENERATED scrub's time with LOCATE
 *             (0.996 - 1.009 of it in mirrored pairs at (10,4), (6,3), (14,32)
 *             and (64,32), inside the run-to-run spread; 1.04 at (13,20) and
 *             (13,24)), ONE_ROW 1.02 - 1.07 of it; against TWO_PASS (10,4) 0.38
 *             / 0.54 ms COLUMNS and 0.40 / 0.60 ONE_ROW, (6,3) 0.40 / 0.63 and
 *             0.43 / 0.70, (14,32) 0.30 / 0.89 and 0.30 / 1.00.  One row of
 *             every block bad in 1 % of the columns, or in all of them: with
 *             e >= 20 0.31 - 0.61 of TWO_PASS in both modes; with e <= 4
 *             COLUMNS 0.83 - 1.02, but ONE_ROW 1.05 - 1.53 (its second launch
 *             runs the whole program again, TWO_PASS only its compare).
 *             Against FUSED at (64,32): 1.29 clean, 2.1 - 2.8 damaged.
 *             So: GENERATED for a matrix without a compiled kernel when most
 *             blocks are clean (what a scrub finds), in COLUMNS mode at any
 *             damage, and at e >= 20 in either mode; ONE_ROW at small e on
 *             heavily damaged data is better left on TWO_PASS, and the
 *             compiled codes on FUSED.
 * All argument checks, the UNSUPPORTED cases and the e == 0 / len == 0 paths
 * are the same under every choice.  rsgpu_correct_blocks does not use it. */
#define RSGPU_REPAIR_KERNEL_AUTO 0
#define RSGPU_REPAIR_KERNEL_GENERATED 1
int rsgpu_set_repair_kernel(rsgpu_ctx *ctx, int kernel);

/* ---- correction per byte column of up to two damaged rows ------------------ */

/* rsgpu_repair_blocks in RSGPU_REPAIR_COLUMNS mode corrects a byte column that
 * one row explains; rsgpu_locate_blocks names several rows, but only from the
 * span of all the block's columns and at most min(8, e - 1) of them.  Damage
 * scattered over many rows of a long stripe (bad sectors, torn writes), no
 * column holding more than two bad rows, ends there as PARTIAL or DAMAGED.
 * This call decodes every byte column on its own, with up to t unknown
 * positions.  With s the syndrome column and h_r as rsgpu_locate_blocks
 * defines them (column r of the matrix for a data row, the unit vector of p
 * for parity row k + p), per bad byte column i:
 *
 *   E1 = { r : s = x h_r for some x != 0 }
 *   E2 = { {a, b}, a != b : s = x h_a + y h_b with x != 0 and y != 0 }
 *
 *   |E1| = 1                  corrected in that row, exactly as
 *                             RSGPU_REPAIR_COLUMNS does it
 *   else, when t = 2, E1 is   corrected in both rows: a data row r gets
 *   empty and |E2| = 1        src[r][i] ^= x_r, a parity row k + p gets
 *                             parity[p][i] ^= x_{k+p}; afterwards all syndromes
 *                             of the column are zero
 *   otherwise                 the column stays byte for byte as it was
 *
 * The verdict is that of the definition, per column, for any matrix the call
 * takes: the search covers all (k + e)(k + e - 1) / 2 pairs, and two matching
 * pairs leave the column alone.  With t = 1 the rows written and the report
 * equal those of rsgpu_repair_blocks with RSGPU_REPAIR_COLUMNS
 * (corrected_columns = its repaired_columns, two_row_columns = 0); with t = 2
 * every column COLUMNS corrects is corrected identically, and columns it
 * leaves may be corrected in two rows.  As there, a correction is the
 * explanation with the fewest rows, not a proof: three or more damaged rows
 * in one column can imitate two (or one) and are then "corrected" into a
 * consistent but wrong column.  A matrix whose every e columns of [C | I] are
 * independent (gf_gen_cauchy1_matrix always) has distance e + 1: with e >= 5
 * three damaged rows of a column never look like two or fewer, and such a
 * column is left alone.
 *
 * Report per block, overwritten by every call: status CLEAN, REPAIRED (every
 * bad column corrected), DAMAGED (none corrected) or PARTIAL; `row` is the
 * common row when every corrected column was a one-row correction in the
 * same row, otherwise -1.  Never written: bytes in [len, pitch), any byte of
 * a column that is not bad, any byte of a row that the column's verdict does
 * not name.
 *
 * Layout, `coef` and accepted geometries as rsgpu_repair_blocks: any len, any
 * pitch >= len, any alignment, a custom e x k matrix or NULL.  d_report
 * [blocks] is DEVICE memory, 8-byte aligned.  t is 1 or 2, anything else
 * RSGPU_ERR_ARG.  The matrix must be locatable (rsgpu_scrub_locatable); t = 1
 * needs e >= 3 (COLUMNS' rule); t = 2 needs 5 <= e <= 64: correcting two
 * errors per column while still detecting three takes distance e + 1 >= 2 * 2
 * + 2 = 6, and a lane of the wave holds one syndrome, as in the locate.
 * Otherwise RSGPU_ERR_UNSUPPORTED.  On either error, on null rows or a null or
 * misaligned report, nothing is enqueued and the report is untouched.  e == 0
 * or len == 0: every block CLEAN.  Enqueued on the context's stream, no
 * synchronisation and no host decision between finding and writing; more
 * than 65535 blocks run as consecutive slices.
 *
 * Two forms, chosen by rsgpu_set_correct_kernel (below); AUTO runs TWO_PASS.
 * TWO_PASS: the encode of a slice into the context's scratch
 * (the TWO_PASS scrub's slices, at most 128 MiB of parity), then
 * k_correct_compare, which is k_repair_compare -- a thread ORs the syndromes
 * of 16 columns per 16-byte load, a clean group costs nothing more, a bad
 * column first gets the one-row test -- whose waves take the columns that
 * test leaves one at a time: lane p holds s_p, two parity rows are read off
 * the non-zero syndromes, a data row with a parity row takes one lane per data
 * row, and the k (k - 1) / 2 pairs of data rows are solved from syndromes 0
 * and 1 (the determinant is non-zero for a locatable matrix) and rejected at
 * syndrome 2, 255 of 256 of them, with four reads of an exp table at sums of
 * logarithms laid out per row before the search.  The tables
 * lie in LDS, 4164 bytes per wave, filled by a wave when it meets its first
 * such column.
 * Cost, measured at (64, 32), 1 MB rows, 1024 blocks on one MI355X, one
 * process, medians of 24 runs (profiles/correct): clean blocks
 * with t = 2 34.60 ms, COLUMNS under the TWO_PASS scrub kernel 34.62 ms (ratio
 * over 24 mirrored pairs 0.958 - 1.009, mean 0.999, stdev 0.010: inside the
 * pair's run-to-run spread; the compare kernels 11.82 and 11.80 ms).  One row
 * per block bad in 1 % of the columns: 172.8 ms with t = 2, 173.0 ms with
 * t = 1, all of it COLUMNS' own walk of bad columns, 13.5 ns per bad column
 * over the device.  A column that goes to the pair search costs 10.1 ns over
 * the device, whichever pair explains it: two rows bad in the same 1 % of
 * the columns 276.8 ms, 12 rows with two per column 276.8 ms.  Blocks damaged
 * in most of their columns are the worst case: two whole rows bad 7575 ms.
 * rsgpu_locate_blocks followed by rsgpu_rebuild_blocks took 62.4, 64.5 and
 * 189.1 ms on the one-row, two-row and whole-row damage.  Advice: scrub
 * first; where the damage lies in whole rows, locate and rebuild; take this
 * call for the blocks they give up as DAMAGED, whose damage is scattered.
 * rsgpu_set_scrub_kernel decides one thing for this call: under
 * rsgpu_set_correct_kernel's FUSED, RSGPU_SCRUB_GENERATED selects the form
 * fused into the generated encode for the matrices that are not compiled in
 * (below).  Under AUTO and TWO_PASS it has no influence.
 * Not built: t > 2; e > 64; host-resident blocks. */
typedef struct rsgpu_correct_report {
    unsigned long long bad_columns;       /* before the call */
    unsigned long long corrected_columns; /* columns written, one- and two-row together */
    unsigned long long two_row_columns;   /* of those, columns corrected in two rows */
    int status;                           /* RSGPU_REPAIR_CLEAN / _REPAIRED / _PARTIAL / _DAMAGED */
    int row; /* the one row every corrected column lay in, each a one-row correction; else -1 */
} rsgpu_correct_report;                   /* 32 bytes */

/* len <= RSGPU_MAX_LEN (RSGPU_ERR_ARG beyond it, nothing written). */
int rsgpu_correct_blocks(rsgpu_ctx *ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                         unsigned char *d_src, unsigned char *d_parity,
                         const unsigned char *coef, int t, rsgpu_correct_report *d_report);

/* Kernel of rsgpu_correct_blocks, per context; rows written and reports are
 * the same under every choice, byte for byte.  An unknown value or a null
 * context is RSGPU_ERR_ARG.  All argument checks, the UNSUPPORTED cases (a
 * matrix that is not locatable, t = 1 with e < 3, t = 2 with e outside [5,
 * 64]) and the e == 0 / len == 0 paths come before the choice and do not
 * depend on it.
 *   AUTO      TWO_PASS: the fused form is opt-in.
 *   TWO_PASS  the encode into the scratch, then k_correct_compare.
 *   FUSED     fused into the compiled encode, as the FUSED scrub and repair
 *             are: per slice of at most 65535 blocks one launch of
 *             k_rs_bs_correct, which is k_rs_bs_repair in its COLUMNS mode --
 *             k_rs_bs's accumulation, the stored parity read once and
 *             compared in registers, nothing written for a clean tile -- and
 *             after all slices k_correct_finalise.  No encode is launched, the
 *             parity scratch is neither touched nor grown, the locate tables
 *             are not uploaded.  A dirty tile lays its syndromes into LDS in
 *             four passes; a column one row explains is corrected as COLUMNS
 *             corrects it, and with t = 2 the others go to the wave one at a
 *             time while the pass's syndromes are in LDS: TWO_PASS's search
 *             (two parity rows off the non-zero syndromes; a data row with a
 *             parity row, a lane per data row; the data pairs, a lane per
 *             higher row, solved from syndromes 0 and 1 and screened at
 *             syndrome 2) on the compiled codes' own coefficients 2^(p r), so
 *             nothing of the matrix is read from memory.  Its tables (the
 *             field's logarithms, 1.3 KB per workgroup; 8 bytes per data row
 *             and 64 per wave) lie in the encode's 32 KB of LDS; no kernel has
 *             scratch, each runs at its k_rs_bs_repair sibling's waves per
 *             SIMD, no plan is left out (profiles/correct_fused).
 *             Measured at (64, 32), 1 MB rows, 1024 blocks on one MI355X, one
 *             process, medians of 24 runs (profiles/correct_fused, DESIGN.md
 *             3.10): clean blocks 22.10 ms, rsgpu_repair_blocks COLUMNS under
 *             the FUSED scrub kernel 21.55 ms (ratio over 24 mirrored pairs
 *             0.876 - 1.054, mean 1.011, stdev 0.035: inside the pair's
 *             run-to-run spread), TWO_PASS 36.09 ms.  One row per block bad
 *             in 1 % of the columns 33.92 ms, a second row bad in the same
 *             columns 108.72 ms, 12 rows with two per column 108.72 ms
 *             (1.15 ns per one-row column and 7.31 ns per pending
 *             column over the device); two whole rows bad 4796 ms
 *             (TWO_PASS 7566 ms in the same process).  At the scrub's
 *             price on clean blocks this call with t = 2 can be the scrub
 *             pass itself; whole damaged rows still belong to
 *             rsgpu_locate_blocks and rsgpu_rebuild_blocks.
 *             Where the FUSED scrub's kernels apply: the compiled codes (16,4)
 *             (16,8) (64,32) (64,16) (100,20) (5,4) (20,7) without `coef`,
 *             pitch % 16 == 0, 16-byte aligned d_src and d_parity, len % 32 ==
 *             0, len < 4 GiB -- so t = 2 on (16,8) (20,7) (64,16) (64,32)
 *             (100,20), t = 1 on those and on (16,4) (5,4).
 *             Otherwise, when the context's scrub kernel is
 *             RSGPU_SCRUB_GENERATED (rsgpu_set_scrub_kernel: the family's
 *             opt-in to the generated programs), fused into the generated
 *             encode: any matrix, with or without `coef`, for e <= 64, 16-byte
 *             aligned rows (pitch % 16 == 0), len % 32 == 0 and len < 4 GiB, on
 *             a device with an executable memory pool.  Per slice one launch of
 *             k_rs_jit_correct (e <= 16) or k_rs_jitw_correct (both recorded as
 *             k_rs_jit_correct) on the matrix's shared program, which is the
 *             GENERATED repair's kernel in its COLUMNS mode -- the stored
 *             parity compared in registers, nothing written for a clean
 *             workgroup -- then k_correct_finalise; no encode, no parity
 *             scratch.  A dirty workgroup lays its syndromes into LDS in eight
 *             passes of 256 columns per tile; a column one row explains is
 *             corrected as COLUMNS corrects it, and with t = 2 the others go to
 *             their wave one at a time while the pass's syndromes are in LDS:
 *             TWO_PASS's search on the matrix read from memory, rows 0 to 2 of
 *             it kept as logarithms in LDS (3 k bytes per workgroup, beside the
 *             field's 1.3 KB; 8 k bytes per wave for the rows of a column).
 *             Those tables share the encode's chunk buffers with the
 *             syndromes.  They fit for every k + e <= 250 in every layout but
 *             the four waves of 16 rows (48 < e <= 64), which take t = 2 while
 *             256 e + 32 k <= 21240: every k up to e = 59, k <= 151 at e = 64;
 *             beyond that t = 2 falls back to TWO_PASS (t = 1 never does).  No
 *             kernel has scratch, each runs at its k_rs_jit_repair /
 *             k_rs_jitw_repair sibling's waves per SIMD
 *             (profiles/correct_generated).  Its times are not measured yet.
 *             Hot path and clean exit are the GENERATED repair's, so clean
 *             blocks should cost what its COLUMNS mode costs; the eight-pass
 *             cold path is small code, not fast code, and loses to TWO_PASS on
 *             damaged blocks at small e in the generated locate and repair
 *             (profiles/locate_generated, profiles/repair_generated): expect
 *             the same here, and take this form for scrub passes over mostly
 *             clean blocks.
 *             The compiled form has precedence where both apply; under any
 *             other scrub kernel FUSED falls back to TWO_PASS for a matrix that
 *             is not compiled in.
 * A choice that does not apply falls back to TWO_PASS, silently. */
#define RSGPU_CORRECT_AUTO 0
#define RSGPU_CORRECT_TWO_PASS 1
#define RSGPU_CORRECT_FUSED 2
int rsgpu_set_correct_kernel(rsgpu_ctx *ctx, int kernel);

/* ---- partial-stripe update: parity follows a few overwritten rows -------- */

#define RSGPU_UPDATE_NONE 255 /* list padding: no row in this slot */
#define RSGPU_UPDATE_DELTA 1  /* flags: d_upd rows are deltas (new ^ old), not new contents */

/* The batched, device-resident form of ec_encode_data_update above: the
 * caller overwrites some of a block's k source rows and the e parity rows
 * follow.  Layout, `coef` and accepted geometries as rsgpu_encode_blocks (any
 * len, any pitch >= len, any alignment, custom e x k matrix or NULL).
 *   d_cols  DEVICE [blocks][u] bytes, 1 <= u <= k: block b's list of source
 *           row indices in [0, k), strictly ascending, then zero or more
 *           RSGPU_UPDATE_NONE to the end (an all-NONE list: the block is not
 *           touched, status 0)
 *   d_upd   DEVICE [blocks][u] rows at `pitch`: slot i belongs to
 *           d_cols[b][i]; slots whose entry is NONE are never read
 * With delta_i the delta of slot i and j_i its row, block b receives
 *   parity[b][p][x] ^= XOR_i c[p][j_i] * delta_i[x]     for p < e, x < len
 *   default flags       delta_i = upd_i ^ src[b][j_i], and src[b][j_i] = upd_i
 *   RSGPU_UPDATE_DELTA  delta_i = upd_i; d_src is neither read nor written
 *                       and may be NULL
 * The syndromes of the block (see the scrub above) are unchanged by the call
 * (with RSGPU_UPDATE_DELTA: by the call together with the caller's own
 * src[b][j_i] ^= delta_i): a consistent block stays consistent, and a block
 * with damage keeps exactly its scrub verdict.
 *
 * d_status[b] (DEVICE, required) = 0, or -2 for a malformed list (not
 * strictly ascending, an index >= k other than NONE, a row after a NONE).
 * The list is validated before any byte of the block is written: a -2 block
 * is not touched at all.  Bytes in [len, pitch), source rows not listed and
 * every byte of d_upd and d_cols are never written.  d_upd must not overlap
 * d_src or d_parity (RSGPU_ERR_ARG).
 *
 * Enqueued on the context's stream, no synchronisation; more than 65535
 * blocks run as consecutive slices.  e == 0 only replaces source rows (and
 * does nothing with RSGPU_UPDATE_DELTA); len == 0 only writes the statuses.
 * Null required pointers, u out of range or unknown flag bits: RSGPU_ERR_ARG,
 * nothing enqueued.
 *
 * Cost (k_update_blocks): every d_upd byte and old source byte is read once,
 * every new source byte written once, and the parity is read and written once
 * per group of 8 listed rows, ceil(n / 8) times for a list of n rows: about
 * (3 n + 2 e ceil(n / 8)) len bytes per block, (n + 2 e ceil(n / 8)) len with
 * RSGPU_UPDATE_DELTA.  Advice to callers, measured at (64, 32), 1 MB rows,
 * 1024 blocks on one MI355X (profiles/update): one row per block takes
 * 12.5 ms against 21.5 ms for rsgpu_encode_blocks of the same blocks; the
 * update beats "copy the new rows in, then re-encode" up to 8 rows per block
 * (17.1 against 24.9 ms) and loses from 9 rows on (29.5 against 25.3 ms),
 * where the second walk over the parity starts.  For another geometry compare
 * the bytes: 3 n + 2 e ceil(n / 8) rows against k + e + 2 n.
 * len <= RSGPU_MAX_LEN (RSGPU_ERR_ARG beyond it, nothing written). */
int rsgpu_update_blocks(rsgpu_ctx *ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                        int u, const unsigned char *d_cols, const unsigned char *d_upd,
                        unsigned char *d_src, unsigned char *d_parity,
                        const unsigned char *coef, int flags, int *d_status);

/* ---- host-resident blocks (the reference's buffers, isa.cpp:46-58) ------- */

/* Page-locked host memory for the host-resident calls: their copies then run
 * as DMA at the link rate and overlap the kernels (pageable memory works,
 * but is copied synchronously, so the stages run in series). */
int rsgpu_host_alloc(rsgpu_ctx *ctx, void **hptr, size_t bytes);
int rsgpu_host_free(rsgpu_ctx *ctx, void *hptr);

/* isa_encoder::encode_all over blocks held in HOST memory, as isa.cpp:46-58
 * holds them (isa.cpp:69-79): h_src [blocks][k] rows, h_parity [blocks][e]
 * rows, at `pitch` >= len.  The batch streams through device staging in
 * chunks, copy-in / rsgpu_encode_blocks / copy-out of consecutive chunks
 * overlapped on three streams.  Synchronous: the parity is in h_parity on
 * return.  `coef` as rsgpu_encode_blocks.  In host memory the call writes
 * bytes [0, len) of each row of h_parity and nothing else, whatever the
 * pitch: bytes in [len, pitch) of any row are never written, nor is any byte
 * of h_src.
 * len <= RSGPU_MAX_LEN (RSGPU_ERR_ARG beyond it, nothing written). */
int rsgpu_encode_blocks_host(rsgpu_ctx *ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                             const unsigned char *h_src, unsigned char *h_parity,
                             const unsigned char *coef);

/* isa_decoder::decode_all over HOST-resident blocks (isa.cpp:169-213): the
 * erasure lists h_err [blocks][e] as rsgpu_decode_blocks; only what the
 * reference's decoder reads crosses the link towards the GPU -- the surviving
 * originals (as runs of consecutive rows; rows shorter than 64 KiB go as
 * whole blocks, erased rows included, which the kernels never read) and the
 * parity rows -- and the recovered rows land in h_out [blocks][e] (in h_err
 * order).  h_status [blocks] (may be NULL) receives rsgpu_decode_blocks'
 * per-block status.  Pipelined and synchronous as rsgpu_encode_blocks_host.
 * In host memory the call writes bytes [0, len) of each of the blocks x e
 * rows of h_out and `blocks` ints of h_status, and nothing else: bytes in
 * [len, pitch) of any row are never written, nor is any byte of h_src,
 * h_parity or h_err, or any int of h_status beyond `blocks`.  A block with a
 * non-zero status has unspecified bytes only in [0, len) of its own rows of
 * h_out.
 * len <= RSGPU_MAX_LEN (RSGPU_ERR_ARG beyond it, nothing written). */
int rsgpu_decode_blocks_host(rsgpu_ctx *ctx, int k, int e, size_t len, size_t pitch, size_t blocks,
                             const unsigned char *h_src, const unsigned char *h_parity,
                             const unsigned char *h_err, unsigned char *h_out, int *h_status);

/* ---- synthetic workload (replaces rand(), isa.cpp:56-58, :137-146) ------- */

/* Fills `rows` rows of `len` bytes at `pitch` with the seeded counter-based
 * stream: bytes 8w..8w+7 of global row (row0 + r) = LE(mix(seed, row, w)). */
int rsgpu_fill_synthetic(rsgpu_ctx *ctx, unsigned char *d_rows, size_t rows, size_t len,
                         size_t pitch, uint64_t seed, uint64_t row0);

/* Host: erasure lists of blocks blk0..blk0+blocks-1 into h_err[blocks][e]
 * (e distinct originals per block, ascending), as the isa_decoder ctor draws
 * them (isa.cpp:137-153) with a seeded generator. */
int rsgpu_erasure_patterns(uint64_t seed, uint64_t blk0, size_t blocks, int k, int e,
                           unsigned char *h_err);

#ifdef __cplusplus
}
#endif

#endif /* RSGPU_H */
