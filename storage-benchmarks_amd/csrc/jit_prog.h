// jit_prog.h -- host-built generated code for a coefficient matrix shared by
// every block (the runtime-coefficient encode: caller `coef`, Cauchy,
// ec_encode_data's gftbls, codes without a compile-time kernel).
//
// The code runs in k_rs_jit (rs_jit.hip) exactly like the per-block decode
// code, with the register contract of rs_jit.h, but each (wave, source)
// preamble builds only the composites its 64 masks need: a greedy cover
// (the algorithm of gen_enc_progs.py, which serves the compile-time encode)
// picks XORs of 2 or 3 available values until every mask is the XOR of at
// most two values, so the multiply-accumulate stays one instruction per
// output plane.  13.4 composites per source for random coefficients against
// the 22 of the full four-Russians tables; when a cover would need more than
// 22, the full tables serve.  Everything here runs on the host: the matrix
// is known there, and the code is built once per matrix and cached.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

namespace rsgpu {
namespace jit {

constexpr int kMaxComposites = 22;  // v32..v53
constexpr uint8_t kNone = 255;

constexpr int kMaxSlots = 16;       // rows per wave: 8 (k_rs_jit), up to 16 (k_rs_jitw)

// One (wave, source) program: value ids 0..7 are the source's planes
// (bit i of a mask = plane i), 8 + i the composite ops[i] = XOR of its 2 or 3
// operand values; accumulator plane b of slot s gets outs[8 s + b] (0, 1 or
// 2 values) XORed in.
struct SrcProg {
    int nops = 0;
    uint8_t ops[kMaxComposites][3];
    uint8_t outs[8 * kMaxSlots][2];
};

// Cover of the masks of coefficients coef[0..nslot-1] (slot s = output row
// R w + s of the wave), nslot <= kMaxSlots.
void plan_source(const uint8_t* coef, int nslot, SrcProg& p, int max_ops = kMaxComposites);

// Largest chunk (8 sources, 8 slots, kMaxComposites 3-input composites),
// rounded to 64-byte lines: the stride between chunks of host-built code.
int host_chunk_stride();

// Code of one chunk (nt <= 8 sources with programs progs[0..nt-1], nslot <=
// 8 slots) at dst; returns its size in bytes (<= host_chunk_stride()).
size_t emit_chunk(uint8_t* dst, int nt, int nslot, const SrcProg* progs);

// The whole program of an e x k matrix c (row-major) in passes of <= 32
// rows: pass p, wave w, chunk ch at ((p NW_MAX + w) nch + ch) stride, with
// NW_MAX = 4 wave slots reserved per pass.  Returns the bytes.
// max_ops < kMaxComposites caps the greedy cover (tests use it to exercise
// the full-table fallback).
std::vector<uint8_t> build_matrix_code(const uint8_t* c, int k, int e, int* chunk_stride,
                                       int max_ops = kMaxComposites);

// The same in the two-wave layout of k_rs_jitw (rs_jit.h Wide<R, CS>, the
// register contract of the decode: planes v10..v17, composites v18..v39,
// accumulators from v40, LDS address in v9) for 16 < e <= 32: wave w (rows
// R w .. R w + R - 1), chunk ch of CS sources at (w nch + ch) stride, each
// source loading its own planes, then its covered composites and one
// instruction per nonzero output mask.  *chunk_stride = the largest chunk
// rounded to 64 bytes.
std::vector<uint8_t> build_matrix_code_wide(const uint8_t* c, int k, int e, int R, int CS, int* chunk_stride,
                                            int max_ops = kMaxComposites);

// Rows of any count the wide layout takes (16 < e <= 125): passes of <= 64
// rows (rs_jit.h wide_passes), each built as above in the layout of its own
// row count (jitw_rows / jitw_cs) and appended; passes[p] = (byte offset of
// pass p, its chunk stride).  Empty when a pass fits no layout.  The
// GENERATED encode's shared programs (rsgpu_capi.cpp shared_program) are
// exactly this.
std::vector<uint8_t> build_matrix_code_wide_passes(const uint8_t* c, int k, int e,
                                                   std::vector<std::pair<size_t, int>>* passes,
                                                   int max_ops = kMaxComposites);

// ---- the Karatsuba-split program of the (64, 32) gf_gen_rs_matrix code ------
//
// V[r][j] = 2^(r j) = D1[r] h(r + j) d[j] with h(n) = 2^C(n, 2), d[j] =
// 2^-C(j, 2), D1[r] = 2^-C(r, 2) (tools/karatsuba_price.py).  One Karatsuba
// level on both 32-source halves (base = 0, 32; q, r < 16; s = 16 (base / 32)
// + q names the source pair x[base + q], x[base + 16 + q]) gives three 16 x 32
// products, one per role wave of a column tile (k_rs_kara, rs_jit.hip):
//   P   over the virtual sources v_s = x[base + q] ^ rho[s] x[base + 16 + q]
//   Q1  over x[base + q],   Q2 over x[base + 16 + q]
//   y[r] = P[r] ^ Q1[r],    y[16 + r] = sigma[r] P[r] ^ Q2[r]
// Code: role w (0 = P, 1 = Q1, 2 = Q2), chunk ch at (w kKaraChunks + ch)
// chunk_stride, in the Wide<16, .> register contract (rs_jit.h).  Chunks 0 ..
// kKaraSrcChunks - 1 hold kKaraPairs source pairs each, pair i of a chunk at
// LDS positions 2 i (x[base + q]) and 2 i + 1 (x[base + 16 + q]); P loads
// both, the second into v18..v25, XORs rho's program (temporaries from v26)
// into v10..v17 and goes on as any source.  Chunk kKaraSrcChunks is the
// combine, run once per tile after the last source chunk: its 16 sources are
// P's rows as planes in LDS (row r at position r), added into slot r through
// the identity (Q1) or sigma[r]'s XOR program (Q2); P's is a bare return.
// (kKaraPairs, kKaraSrcChunks, kKaraChunks, kara_source: rs_jit.h, shared
// with the kernel.)
struct KaraProgram {
    std::vector<uint8_t> code;
    int chunk_stride = 0;
    uint8_t cP[16 * 32], cQ1[16 * 32], cQ2[16 * 32];  // [r][s]
    uint8_t rho[32], sigma[16];
};

// Builds the program for the 32 x 64 matrix c (row-major), which must be the
// gf_gen_rs_matrix parity rows: every coefficient of c is checked against the
// split, and false comes back (nothing built) when one differs or a scaling
// program needs more temporaries than the contract has.
bool build_karatsuba_code(const uint8_t* c, KaraProgram* out);

}  // namespace jit
}  // namespace rsgpu
