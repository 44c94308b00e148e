// jit_prog.cpp -- host-built generated code for a shared coefficient matrix
// (jit_prog.h).  Instruction encodings and the register contract: rs_jit.h.
#include "jit_prog.h"

#include <string.h>

#include <algorithm>

#include "rs_jit.h"
#include "rs_kernels.h"

namespace rsgpu {
namespace jit {

namespace {

// value id -> VGPR for a source in plane bank `bank`
inline int value_reg(int v, int bank) { return v < 8 ? plane_reg(bank, v) : 32 + (v - 8); }

// The full four-Russians tables (L[n] over planes 0-3, H[n] over 4-7, the 22
// composites of rs_jit.h's fixed layout) as a program: always a cover.
void full_tables(const uint8_t (&masks)[8 * kMaxSlots], int nm, SrcProg& p)
{
    uint8_t id[256];
    memset(id, kNone, sizeof id);
    for (int a = 0; a < 8; ++a)
        id[1 << a] = (uint8_t)a;
    p.nops = 0;
    for (int hi = 0; hi < 2; ++hi)
        for (int n = 1; n < 16; ++n) {
            const int low = n & -n;
            if (n == low)
                continue;
            const int sh = 4 * hi;
            p.ops[p.nops][0] = id[(n ^ low) << sh];
            p.ops[p.nops][1] = id[low << sh];
            p.ops[p.nops][2] = kNone;
            id[n << sh] = (uint8_t)(8 + p.nops);
            ++p.nops;
        }
    for (int i = 0; i < nm; ++i) {
        const int lo = masks[i] & 15, hi = masks[i] & 0xF0;
        p.outs[i][0] = lo ? id[lo] : (hi ? id[hi] : kNone);
        p.outs[i][1] = (lo && hi) ? id[hi] : kNone;
    }
}

}  // namespace

void plan_source(const uint8_t* coef, int nslot, SrcProg& p, int max_ops)
{
    uint8_t masks[8 * kMaxSlots];
    const int nm = 8 * nslot;
    for (int s = 0; s < nslot; ++s)
        for (int b = 0; b < 8; ++b)
            masks[8 * s + b] = mat_row(coef[s], b);
    // greedy cover (gen_enc_progs.py program()): values available so far,
    // have[m] = value id of mask m
    uint8_t have[256];
    memset(have, kNone, sizeof have);
    uint8_t vals[8 + kMaxComposites];
    int nv = 0;
    for (int a = 0; a < 8; ++a) {
        vals[nv] = (uint8_t)(1 << a);
        have[1 << a] = (uint8_t)nv++;
    }
    auto in = [&](int m) { return m == 0 || have[m] != kNone; };
    auto covered = [&](int m) {
        if (m == 0 || have[m] != kNone)
            return true;
        for (int i = 0; i < nv; ++i)
            if (have[m ^ vals[i]] != kNone)
                return true;
        return false;
    };
    bool need[256] = {};
    for (int i = 0; i < nm; ++i)
        if (!covered(masks[i]))
            need[masks[i]] = true;
    p.nops = 0;
    bool over = false;
    for (;;) {
        int nneed = 0;
        uint8_t nl[256];
        for (int m = 1; m < 256; ++m)
            if (need[m])
                nl[nneed++] = (uint8_t)m;
        if (!nneed)
            break;
        if (p.nops == max_ops || p.nops == kMaxComposites) {
            over = true;
            break;
        }
        bool cand[256] = {};
        for (int i = 0; i < nneed; ++i) {
            cand[nl[i]] = true;  // x ^ 0
            for (int j = 0; j < nv; ++j)
                cand[nl[i] ^ vals[j]] = true;
        }
        int best = -1, best_n = -1;
        uint8_t best_src[3] = {kNone, kNone, kNone};
        for (int c = 1; c < 256; ++c) {
            if (!cand[c] || have[c] != kNone)
                continue;
            uint8_t src[3] = {kNone, kNone, kNone};
            bool ok = false;
            for (int j = 0; j < nv && !ok; ++j) {  // one 2-input XOR of available values
                const int r = c ^ vals[j];
                if (r && have[r] != kNone) {
                    src[0] = (uint8_t)j;
                    src[1] = have[r];
                    ok = true;
                }
            }
            for (int j = 0; j < nv && !ok; ++j)  // or one 3-input XOR
                for (int l = j + 1; l < nv && !ok; ++l) {
                    const int r = c ^ vals[j] ^ vals[l];
                    if (r && r != vals[j] && r != vals[l] && have[r] != kNone) {
                        src[0] = (uint8_t)j;
                        src[1] = (uint8_t)l;
                        src[2] = have[r];
                        ok = true;
                    }
                }
            if (!ok)
                continue;
            int n = 0;
            for (int i = 0; i < nneed; ++i)
                n += nl[i] == c || in(nl[i] ^ c);
            if (n > best_n) {
                best = c;
                best_n = n;
                memcpy(best_src, src, 3);
            }
        }
        if (best < 0) {  // nothing buildable helps: fall back to the full tables
            over = true;
            break;
        }
        memcpy(p.ops[p.nops], best_src, 3);
        ++p.nops;
        vals[nv] = (uint8_t)best;
        have[best] = (uint8_t)nv++;
        for (int i = 0; i < nneed; ++i)
            if (covered(nl[i]))
                need[nl[i]] = false;
    }
    if (over) {
        full_tables(masks, nm, p);
        return;
    }
    for (int i = 0; i < nm; ++i) {
        const int m = masks[i];
        p.outs[i][0] = p.outs[i][1] = kNone;
        if (m == 0)
            continue;
        if (have[m] != kNone) {
            p.outs[i][0] = have[m];
            continue;
        }
        for (int j = 0; j < nv; ++j)
            if (have[m ^ vals[j]] != kNone) {
                p.outs[i][0] = (uint8_t)j;
                p.outs[i][1] = have[m ^ vals[j]];
                break;
            }
    }
}

int host_chunk_stride()
{
    const int per_src = 16 + 4 + 8 * kMaxComposites + 64 * 8;
    return (PRO_BYTES + 8 * per_src + EPI_BYTES + 63) / 64 * 64;
}

size_t emit_chunk(uint8_t* dst, int nt, int nslot, const SrcProg* progs)
{
    size_t o = 0;
    auto put32 = [&](uint32_t w) {
        memcpy(dst + o, &w, 4);
        o += 4;
    };
    auto put64 = [&](uint64_t w) {
        memcpy(dst + o, &w, 8);
        o += 8;
    };
    put64(enc_ds_read_b128(plane_reg(0, 0), 20, 0));
    put64(enc_ds_read_b128(plane_reg(0, 4), 20, LDS_HALF));
    for (int t = 0; t < nt; ++t) {
        const int bank = t & 1, nb = bank ^ 1;
        if (t + 1 < nt) {  // the next source's planes into the other bank
            put64(enc_ds_read_b128(plane_reg(nb, 0), 20, (t + 1) * LDS_SRC));
            put64(enc_ds_read_b128(plane_reg(nb, 4), 20, (t + 1) * LDS_SRC + LDS_HALF));
            put32(enc_waitcnt_lgkm(2));  // this source's two loads done
        } else {
            put32(enc_waitcnt_lgkm(0));
        }
        const SrcProg& p = progs[t];
        for (int i = 0; i < p.nops; ++i) {
            const int d = 32 + i, a = value_reg(p.ops[i][0], bank), b = value_reg(p.ops[i][1], bank);
            if (p.ops[i][2] == kNone)
                put32(enc_xor_e32(d, a, b));
            else
                put64(enc_bitop3_96(d, a, b, value_reg(p.ops[i][2], bank)));
        }
        for (int s = 0; s < nslot; ++s)
            for (int b = 0; b < 8; ++b) {
                const uint8_t* q = p.outs[8 * s + b];
                const int acc = ACC + 8 * s + b;
                if (q[0] == kNone)
                    continue;  // zero mask: nothing to add
                if (q[1] == kNone)
                    put64(enc_xor_e64(acc, acc, value_reg(q[0], bank)));
                else
                    put64(enc_bitop3_96(acc, acc, value_reg(q[0], bank), value_reg(q[1], bank)));
            }
    }
    put64((uint64_t)S_NOP0 << 32 | S_SETPC_82);
    return o;
}

std::vector<uint8_t> build_matrix_code(const uint8_t* c, int k, int e, int* chunk_stride, int max_ops)
{
    const int stride = host_chunk_stride(), nch = (k + 7) / 8, passes = (e + 31) / 32;
    *chunk_stride = stride;
    std::vector<uint8_t> code((size_t)passes * 4 * nch * stride);
    // unused bytes: returns (a call that lands there comes straight back)
    for (size_t i = 0; i + 8 <= code.size(); i += 8) {
        const uint64_t ret = (uint64_t)S_NOP0 << 32 | S_SETPC_82;
        memcpy(&code[i], &ret, 8);
    }
    SrcProg progs[8];
    for (int p = 0; p < passes; ++p) {
        const int rows = std::min(32, e - 32 * p), nw = (rows + 7) / 8;
        for (int w = 0; w < nw; ++w) {
            const int nslot = std::min(8, rows - 8 * w);
            for (int ch = 0; ch < nch; ++ch) {
                const int nt = std::min(8, k - 8 * ch);
                for (int t = 0; t < nt; ++t) {
                    uint8_t cf[8];
                    for (int s = 0; s < nslot; ++s)
                        cf[s] = c[(size_t)(32 * p + 8 * w + s) * k + 8 * ch + t];
                    plan_source(cf, nslot, progs[t], max_ops);
                }
                emit_chunk(&code[(((size_t)p * 4 + w) * nch + ch) * stride], nt, nslot, progs);
            }
        }
    }
    return code;
}

namespace {

// value id -> VGPR in the two-wave layout (rs_jit.h Wide)
inline int wide_reg(int v) { return v < 8 ? 10 + v : 18 + (v - 8); }

// Code bytes appended at dst (nullptr: size only)
struct Writer {
    uint8_t* dst;
    size_t o = 0;
    void put32(uint32_t w)
    {
        if (dst)
            memcpy(dst + o, &w, 4);
        o += 4;
    }
    void put64(uint64_t w)
    {
        if (dst)
            memcpy(dst + o, &w, 8);
        o += 8;
    }
};

// A source's planes from LDS position `pos` into v[first .. first + 7]
void emit_load_planes(Writer& w, int first, int pos)
{
    w.put64(enc_ds_read_b128(first, 9, pos * LDS_SRC));
    w.put64(enc_ds_read_b128(first + 4, 9, pos * LDS_SRC + LDS_HALF));
}

// The covered composites of p from the planes in v10..v17, then one
// instruction per nonzero output mask of the nslot slots
void emit_source_body(Writer& w, int nslot, const SrcProg& p)
{
    for (int i = 0; i < p.nops; ++i) {
        const int d = 18 + i, a = wide_reg(p.ops[i][0]), b = wide_reg(p.ops[i][1]);
        if (p.ops[i][2] == kNone)
            w.put32(enc_xor_e32(d, a, b));
        else
            w.put64(enc_bitop3_96(d, a, b, wide_reg(p.ops[i][2])));
    }
    for (int s = 0; s < nslot; ++s)
        for (int b = 0; b < 8; ++b) {
            const uint8_t* q = p.outs[8 * s + b];
            const int acc = 40 + 8 * s + b;
            if (q[0] == kNone)
                continue;  // zero mask: nothing to add
            if (q[1] == kNone)
                w.put64(enc_xor_e64(acc, acc, wide_reg(q[0])));
            else
                w.put64(enc_bitop3_96(acc, acc, wide_reg(q[0]), wide_reg(q[1])));
        }
}

// One chunk of the two-wave layout at dst (nullptr: size only).
size_t emit_chunk_wide(uint8_t* dst, int nt, int nslot, const SrcProg* progs)
{
    Writer w{dst};
    for (int t = 0; t < nt; ++t) {
        emit_load_planes(w, 10, t);
        w.put32(enc_waitcnt_lgkm(0));
        emit_source_body(w, nslot, progs[t]);
    }
    w.put64((uint64_t)S_NOP0 << 32 | S_SETPC_82);
    return w.o;
}

}  // namespace

std::vector<uint8_t> build_matrix_code_wide(const uint8_t* c, int k, int e, int R, int CS, int* chunk_stride,
                                            int max_ops)
{
    const int nch = (k + CS - 1) / CS;
    // programs of every (wave, source), then the chunk sizes
    const int nv = wide_waves(e);
    auto row0 = [&](int w) { return wide_row0(e, w); };
    if ((e + nv - 1) / nv > R || R > kMaxSlots)  // a wave's rows exceed its accumulators
        return {};
    std::vector<SrcProg> progs((size_t)nv * k);
    for (int w = 0; w < nv; ++w) {
        const int nslot = row0(w + 1) - row0(w);
        for (int q = 0; q < k && nslot > 0; ++q) {
            uint8_t cf[kMaxSlots];
            for (int s = 0; s < nslot; ++s)
                cf[s] = c[(size_t)(row0(w) + s) * k + q];
            plan_source(cf, nslot, progs[(size_t)w * k + q], max_ops);
        }
    }
    size_t most = 0;
    for (int w = 0; w < nv; ++w) {
        const int nslot = row0(w + 1) - row0(w);
        for (int ch = 0; ch < nch && nslot > 0; ++ch)
            most = std::max(most, emit_chunk_wide(nullptr, std::min(CS, k - CS * ch), nslot,
                                                  &progs[(size_t)w * k + CS * ch]));
    }
    const int stride = (int)((most + 63) / 64 * 64);
    *chunk_stride = stride;
    std::vector<uint8_t> code((size_t)nv * nch * stride);
    for (size_t i = 0; i + 8 <= code.size(); i += 8) {
        const uint64_t ret = (uint64_t)S_NOP0 << 32 | S_SETPC_82;
        memcpy(&code[i], &ret, 8);
    }
    for (int w = 0; w < nv; ++w) {
        const int nslot = row0(w + 1) - row0(w);
        for (int ch = 0; ch < nch && nslot > 0; ++ch)
            emit_chunk_wide(&code[((size_t)w * nch + ch) * stride], std::min(CS, k - CS * ch), nslot,
                            &progs[(size_t)w * k + CS * ch]);
    }
    return code;
}

std::vector<uint8_t> build_matrix_code_wide_passes(const uint8_t* c, int k, int e,
                                                   std::vector<std::pair<size_t, int>>* passes, int max_ops)
{
    std::vector<uint8_t> code;
    passes->clear();
    for (int p = 0; p < wide_passes(e); ++p) {
        const int r0 = wide_pass_row0(e, p), pr = wide_pass_rows(e, p);
        int stride = 0;
        const std::vector<uint8_t> cp =
            build_matrix_code_wide(c + (size_t)r0 * k, k, pr, jitw_rows(pr), jitw_cs(pr), &stride, max_ops);
        if (cp.empty())
            return {};
        passes->push_back({code.size(), stride});
        code.insert(code.end(), cp.begin(), cp.end());
    }
    return code;
}

// ---- the Karatsuba-split (64, 32) program (jit_prog.h) ----------------------
namespace {

uint8_t gf_mul(uint8_t a, uint8_t b)
{
    uint8_t r = 0;
    for (; b; b >>= 1) {
        if (b & 1)
            r ^= a;
        a = (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1D : 0));
    }
    return r;
}

uint8_t gf_pow2(int n)  // 2^n, any sign
{
    n = ((n % 255) + 255) % 255;
    uint8_t v = 1;
    for (int i = 0; i < n; ++i)
        v = gf_mul(v, 2);
    return v;
}

uint8_t gf_inv(uint8_t c)
{
    for (int n = 0; n < 255; ++n)
        if (gf_mul(c, gf_pow2(n)) == 1)
            return gf_pow2(n);
    return 0;
}

// XOR program of y -> c y on 8 planes (gen_enc_progs.py twiddle): value ids
// 0..7 the planes of y, 8 + i the XOR of ops[i]'s 2 or 3 values; outs[b] the
// value that is plane b of c y.  Greedy: an output that is one XOR of
// available values is built at once, else the 3-input XOR that brings the
// most outputs within one XOR is added.
struct ScaleProg {
    int nops = 0;
    uint8_t ops[40][3];
    uint8_t outs[8];
};

bool plan_scale(uint8_t c, ScaleProg& p)
{
    if (!c)
        return false;
    uint8_t have[256], vals[48];
    memset(have, kNone, sizeof have);
    int nv = 0;
    for (int a = 0; a < 8; ++a) {
        vals[nv] = (uint8_t)(1 << a);
        have[1 << a] = (uint8_t)nv++;
    }
    auto one_op = [&](int m, uint8_t (&src)[3]) {
        for (int i = 0; i < nv; ++i) {
            const int r = m ^ vals[i];
            if (r && have[r] != kNone && have[r] != i) {
                src[0] = (uint8_t)i, src[1] = have[r], src[2] = kNone;
                return true;
            }
        }
        for (int i = 0; i < nv; ++i)
            for (int j = i + 1; j < nv; ++j) {
                const int r = m ^ vals[i] ^ vals[j];
                if (r && have[r] != kNone && have[r] != i && have[r] != j) {
                    src[0] = (uint8_t)i, src[1] = (uint8_t)j, src[2] = have[r];
                    return true;
                }
            }
        return false;
    };
    uint8_t outm[8];
    for (int b = 0; b < 8; ++b)
        outm[b] = mat_row(c, b);
    p.nops = 0;
    for (;;) {
        int need[8], nn = 0;
        for (int b = 0; b < 8; ++b)
            if (have[outm[b]] == kNone && std::find(need, need + nn, (int)outm[b]) == need + nn)
                need[nn++] = outm[b];
        if (!nn)
            break;
        if (p.nops == 32)
            return false;
        int pick = -1;
        uint8_t src[3];
        for (int i = 0; i < nn && pick < 0; ++i)
            if (one_op(need[i], src))
                pick = need[i];
        if (pick < 0) {
            int best_n = -1;
            for (int i = 0; i < nv; ++i)
                for (int j = i + 1; j < nv; ++j)
                    for (int l = j + 1; l < nv; ++l) {
                        const int cnd = vals[i] ^ vals[j] ^ vals[l];
                        if (!cnd || have[cnd] != kNone)
                            continue;
                        vals[nv] = (uint8_t)cnd;
                        have[cnd] = (uint8_t)nv++;
                        int n = 0;
                        uint8_t tmp[3];
                        for (int x = 0; x < nn; ++x)
                            n += one_op(need[x], tmp);
                        have[cnd] = kNone;
                        --nv;
                        if (n > best_n) {
                            best_n = n;
                            pick = cnd;
                            src[0] = (uint8_t)i, src[1] = (uint8_t)j, src[2] = (uint8_t)l;
                        }
                    }
            if (pick < 0)
                return false;
        }
        memcpy(p.ops[p.nops++], src, 3);
        vals[nv] = (uint8_t)pick;
        have[pick] = (uint8_t)nv++;
    }
    for (int b = 0; b < 8; ++b)
        p.outs[b] = have[outm[b]];
    return true;
}

// dst[b] ^= plane b of c y, y's planes in v[ybase .. ybase + 7], temporaries
// from v[tmp0] up to v39: an output that is a 2-input XOR nothing else reads
// takes dst[b] as its third input and no register.  False when the
// temporaries do not fit.
bool emit_scale_add(Writer& w, uint8_t c, int ybase, int tmp0, const int (&dst)[8])
{
    ScaleProg p;
    if (!plan_scale(c, p))
        return false;
    bool read[48] = {}, fused[48] = {};
    for (int i = 0; i < p.nops; ++i)
        for (int j = 0; j < 3; ++j)
            if (p.ops[i][j] != kNone)
                read[p.ops[i][j]] = true;
    for (int b = 0; b < 8; ++b) {
        const int o = p.outs[b];
        if (o >= 8 && !read[o] && p.ops[o - 8][2] == kNone)
            fused[o] = true;
    }
    int reg[48], tmp = tmp0;
    for (int v = 0; v < 8; ++v)
        reg[v] = ybase + v;
    for (int i = 0; i < p.nops; ++i) {
        if (fused[8 + i])
            continue;
        if (tmp > 39)
            return false;
        const int d = reg[8 + i] = tmp++;
        if (p.ops[i][2] == kNone)
            w.put32(enc_xor_e32(d, reg[p.ops[i][0]], reg[p.ops[i][1]]));
        else
            w.put64(enc_bitop3_96(d, reg[p.ops[i][0]], reg[p.ops[i][1]], reg[p.ops[i][2]]));
    }
    for (int b = 0; b < 8; ++b) {
        const int o = p.outs[b];
        if (fused[o])
            w.put64(enc_bitop3_96(dst[b], dst[b], reg[p.ops[o - 8][0]], reg[p.ops[o - 8][1]]));
        else
            w.put64(enc_xor_e64(dst[b], dst[b], reg[o]));
    }
    return true;
}

// One chunk of role `role` of the Karatsuba program at dst (nullptr: size
// only); 0 when a scaling program does not fit its temporaries.
size_t emit_chunk_kara(uint8_t* dst, const KaraProgram& kp, int role, int ch)
{
    Writer w{dst};
    const uint64_t ret = (uint64_t)S_NOP0 << 32 | S_SETPC_82;
    if (ch == kKaraSrcChunks) {  // the combine: P's row r from position r into slot r
        for (int r = 0; r < 16 && role != 0; ++r) {
            emit_load_planes(w, 10, r);
            w.put32(enc_waitcnt_lgkm(0));
            int acc[8];
            for (int b = 0; b < 8; ++b)
                acc[b] = 40 + 8 * r + b;
            if (!emit_scale_add(w, role == 1 ? 1 : kp.sigma[r], 10, 18, acc))
                return 0;
        }
        w.put64(ret);
        return w.o;
    }
    const uint8_t* m = role == 0 ? kp.cP : role == 1 ? kp.cQ1 : kp.cQ2;
    for (int i = 0; i < kKaraPairs; ++i) {
        const int s = kKaraPairs * ch + i;
        if (role == 0) {  // the virtual source: x[base + q] ^ rho x[base + 16 + q]
            emit_load_planes(w, 10, 2 * i);
            emit_load_planes(w, 18, 2 * i + 1);
            w.put32(enc_waitcnt_lgkm(0));
            const int pl[8] = {10, 11, 12, 13, 14, 15, 16, 17};
            if (!emit_scale_add(w, kp.rho[s], 18, 26, pl))
                return 0;
        } else {
            emit_load_planes(w, 10, 2 * i + (role - 1));
            w.put32(enc_waitcnt_lgkm(0));
        }
        uint8_t cf[16];
        for (int r = 0; r < 16; ++r)
            cf[r] = m[r * 32 + s];
        SrcProg prog;
        plan_source(cf, 16, prog);
        emit_source_body(w, 16, prog);
    }
    w.put64(ret);
    return w.o;
}

}  // namespace

bool build_karatsuba_code(const uint8_t* c, KaraProgram* out)
{
    KaraProgram& kp = *out;
    auto c2 = [](int n) { return n * (n - 1) / 2; };
    auto h = [&](int n) { return gf_pow2(c2(n)); };
    uint8_t d[64], D1[32];
    for (int j = 0; j < 64; ++j)
        d[j] = gf_pow2(-c2(j));
    for (int r = 0; r < 32; ++r)
        D1[r] = gf_pow2(-c2(r));
    for (int r = 0; r < 16; ++r)
        kp.sigma[r] = gf_mul(D1[r + 16], gf_inv(D1[r]));
    for (int base = 0; base < 64; base += 32)
        for (int q = 0; q < 16; ++q) {
            const int s = 16 * (base / 32) + q;
            kp.rho[s] = gf_mul(d[base + 16 + q], gf_inv(d[base + q]));
            for (int r = 0; r < 16; ++r) {
                const uint8_t hb = h(r + q + base + 16);
                kp.cP[r * 32 + s] = gf_mul(gf_mul(D1[r], hb), d[base + q]);
                kp.cQ1[r * 32 + s] = gf_mul(gf_mul(D1[r], (uint8_t)(h(r + q + base) ^ hb)), d[base + q]);
                kp.cQ2[r * 32 + s] =
                    gf_mul(gf_mul(D1[r + 16], (uint8_t)(h(r + q + base + 32) ^ hb)), d[base + 16 + q]);
                // the split reproduces all four coefficients of c it stands for
                const uint8_t p = kp.cP[r * 32 + s], pr = gf_mul(p, kp.rho[s]);
                if ((uint8_t)(p ^ kp.cQ1[r * 32 + s]) != c[r * 64 + base + q] || pr != c[r * 64 + base + 16 + q] ||
                    gf_mul(kp.sigma[r], p) != c[(16 + r) * 64 + base + q] ||
                    (uint8_t)(gf_mul(kp.sigma[r], pr) ^ kp.cQ2[r * 32 + s]) != c[(16 + r) * 64 + base + 16 + q])
                    return false;
            }
        }
    size_t most = 0;
    for (int role = 0; role < 3; ++role)
        for (int ch = 0; ch < kKaraChunks; ++ch) {
            const size_t n = emit_chunk_kara(nullptr, kp, role, ch);
            if (!n)
                return false;
            most = std::max(most, n);
        }
    kp.chunk_stride = (int)((most + 63) / 64 * 64);
    kp.code.assign((size_t)3 * kKaraChunks * kp.chunk_stride, 0);
    for (size_t i = 0; i + 8 <= kp.code.size(); i += 8) {
        const uint64_t ret = (uint64_t)S_NOP0 << 32 | S_SETPC_82;
        memcpy(&kp.code[i], &ret, 8);
    }
    for (int role = 0; role < 3; ++role)
        for (int ch = 0; ch < kKaraChunks; ++ch)
            emit_chunk_kara(&kp.code[((size_t)role * kKaraChunks + ch) * kp.chunk_stride], kp, role, ch);
    return true;
}

}  // namespace jit
}  // namespace rsgpu
