// clyread.hip — batched ReadLogRecord by position (include/clyread.h), gfx950.
//
// Reference: getLogRecordByPos (db.go:676-704) = one DataFile.ReadLogRecord
// (data/dataFile.go:64-111) at an arbitrary (fid, offset).  The positions are
// independent, unordered and untrusted, so nothing here relies on records
// lying back to back (k_scan does) or on a plan (k_mcopy does).
//
// Structure: verify, then size, then gather.
//   k_rd_hdr     one lane per position: file lookup (binary search of the
//                fid-sorted table), step_hdr on the clamped header bytes, the
//                tuple, the CRC span [offset+4, offset+size) and the number of
//                64-byte source lines ("pieces") it touches
//   scan         exclusive scan of the piece counts: the flattened piece list
//   k_rd_plan    lists the records whose pieces cross a 64-piece wave boundary
//   k_rd_crc     a wave takes 64 consecutive pieces: every lane runs its
//                masked, aligned 64 B through a slice-by-4 table CRC (LDS,
//                zero initial register); lanes of one record combine by the
//                shift identity reg(A||B) = A^|B| reg(A) ^ reg0(B) in a
//                segmented log-step scan whose x^(8*64*2^k) factors are
//                compile-time; a record inside the wave gets its verdict, a
//                record that leaves the wave one partial register per wave
//   k_rd_finish  one wave per multi-wave record: shifts its partials by the
//                bytes that follow them, XOR-reduces, compares
//   k_rd_vs      final status -> value sizes (0 for a failed CRC), counters
//   scan         exclusive scan of the value sizes: d_val_off
//   k_rd_gather  the piece list again: every lane stores the value part of
//                its 64 source bytes
// No workgroup waits on another: ordering is kernel boundaries on the stream.
// The 0xFFFFFFFF initial register is folded into the expected value once per
// record (k_rd_hdr): want = ~crc ^ A^len 0xFFFFFFFF.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/clyread.h"
#include "scan_core.h"

#define CLY_TAG "clyread"
#include "cly_internal.h"

#define RD_NT 256                 // threads per workgroup (4 waves)
#define RD_IT 8                   // 64-piece groups a wave of k_rd_crc / k_rd_gather takes in turn
#define RD_SAFE_FIRST 1u          // the span's first 64-B line lies wholly inside the file
#define RD_SAFE_LAST 2u           // the span's last 64-B line lies wholly inside the file
#define RD_MAX_FILE_LEN ((1ull << 47) - 1)

struct RdFile { uint64_t base, len; uint32_t fid, _pad; };     // fid-sorted device copy of cly_file
struct RdSpan {                  // per position, 32 B (meaningful while its status is CLY_READ_REC)
    uint64_t p;                  // address of the first CRC'd byte: base + offset + 4
    uint64_t len;                // bytes CRC'd: size - 4 (> 0)
    uint64_t vrel;               // the value's first byte relative to p: header_size - 4 + key_size
    uint32_t want;               // the zero-init register the span must give: ~crc ^ A^len 0xFFFFFFFF
    uint32_t flags;              // RD_SAFE_*
};
struct RdTot { unsigned long long n_rec, n_eof, n_crc, n_other, n_nofile, value_bytes, record_bytes, n_multi; };

// word layout of the constant table (RS_TAB): slice-by-4 tables, then x^(8n), n = 0..64
#define RT_X8 1024
#define RT_WORDS (1024 + 65)

// ---------------------------------------------------------------------------
// GF(2) constants at compile time (the same algebra as crc_gf.h)
static constexpr uint32_t c_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 31; k >= 0; k--) {
        if (a & (1u << k)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ CLY_POLY : b >> 1;
    }
    return p;
}
static constexpr uint32_t c_x8n(uint64_t nbytes) {
    uint32_t p = 1u << 31, sq = 1u << 23;
    while (nbytes) {
        if (nbytes & 1) p = c_mul(sq, p);
        sq = c_mul(sq, sq);
        nbytes >>= 1;
    }
    return p;
}
// a * C mod P with C known at compile time: the loop's b sequence folds to constants
template <uint32_t C>
__device__ __forceinline__ uint32_t mul_const(uint32_t a) {
    uint32_t p = 0, b = C;
#pragma unroll
    for (int k = 31; k >= 0; k--) {
        p ^= (0u - ((a >> k) & 1u)) & b;
        b = (b & 1) ? (b >> 1) ^ CLY_POLY : b >> 1;
    }
    return p;
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(RD_NT) void k_rd_hdr(uint64_t n, const cly_pos* __restrict__ pos,
                                                  const RdFile* __restrict__ files, int nfiles,
                                                  cly_tuple* __restrict__ tuples, int32_t* __restrict__ status,
                                                  RdSpan* __restrict__ span, uint64_t* __restrict__ np) {
    const uint64_t i = (uint64_t)blockIdx.x * RD_NT + threadIdx.x;
    if (i > n) return;
    if (i == n) { np[n] = 0; return; }
    const cly_pos ps = pos[i];
    cly_tuple t;
    t.offset = ps.offset; t.expiration = 0; t.tx_id = 0; t.fid = ps.fid; t.size = 0; t.key_size = 0;
    t.value_size = 0; t.type = 0; t.data_type = 0; t.header_size = 0; t.txid_len = 0; t.crc = 0;
    RdSpan sp;
    sp.p = 0; sp.len = 0; sp.vrel = 0; sp.want = 0; sp.flags = 0;
    uint64_t pieces = 0;
    int32_t st;
    int lo = 0, hi = nfiles;                         // first entry with fid >= ps.fid
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (files[mid].fid < ps.fid) lo = mid + 1; else hi = mid;
    }
    if (lo >= nfiles || files[lo].fid != ps.fid) st = CLY_READ_NOFILE;
    else if (ps.offset < 0) st = CLY_ERR_OFFSET;
    else {
        const RdFile f = files[lo];
        const uint8_t* base = (const uint8_t*)f.base;
        // reads b[0..m), m = min(26, len - offset): nothing past the file
        const Hdr h = step_hdr(base, ps.offset, (int64_t)f.len, ps.offset);
        st = h.status;
        if (h.status == REC_OK) {
            const uint64_t slen = (uint64_t)h.size - 4;
            if (slen == 0) st = CLY_ERR_CRC;         // empty span: CRC 0, and crc == 0 would have been END_ZERO
            else {
                st = CLY_READ_REC;
                t.expiration = h.exp; t.size = (uint32_t)h.size; t.key_size = h.ks; t.value_size = h.vs;
                t.type = (uint8_t)h.type; t.data_type = (uint8_t)h.dt; t.header_size = (uint8_t)h.hsz; t.crc = h.crc;
                int tn;                              // parseLogRecordKey: inside the key, so inside the file
                const int64_t tx = go_varint(base + ps.offset + h.hsz, (int64_t)h.ks, tn);
                if (tn < 0) { t.tx_id = 0; t.txid_len = 0xFF; }
                else { t.tx_id = tx; t.txid_len = (uint8_t)tn; }
                sp.p = f.base + (uint64_t)ps.offset + 4;
                sp.len = slen;
                sp.vrel = (uint64_t)h.hsz - 4 + h.ks;
                sp.want = ~h.crc ^ cly_shift(0xFFFFFFFFu, slen);
                const uint64_t l0 = sp.p & ~63ull, l1 = (sp.p + slen - 1) & ~63ull;
                if (l0 >= f.base) sp.flags |= RD_SAFE_FIRST;
                if (l1 + 64 <= f.base + f.len) sp.flags |= RD_SAFE_LAST;
                pieces = ((l1 - l0) >> 6) + 1;
            }
        }
    }
    status[i] = st;
    span[i] = sp;
    np[i] = pieces;
    if (tuples) tuples[i] = t;
}

// Records whose pieces [pofs[i], pofs[i+1]) cross a multiple of 64: k_rd_crc
// leaves partials for them, k_rd_finish takes one wave each.
__global__ __launch_bounds__(RD_NT) void k_rd_plan(uint64_t n, const uint64_t* __restrict__ pofs,
                                                   uint64_t* __restrict__ multi, RdTot* __restrict__ tot) {
    const uint64_t i = (uint64_t)blockIdx.x * RD_NT + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = pofs[i], e = pofs[i + 1];
    if (e > s && (s >> 6) != ((e - 1) >> 6)) multi[atomicAdd(&tot->n_multi, 1ull)] = i;
}

// The piece a lane owns: its record and the bytes of its 64-B source line.
struct Piece {
    uint64_t rec, s, e;          // record, its piece range
    uint64_t line;               // 64-B aligned source address
    int lo, hi;                  // the span's bytes of the line: [lo, hi), 0 <= lo < hi <= 64
    bool safe;                   // the whole line may be loaded
    RdSpan sp;
};
__device__ __forceinline__ Piece locate(uint64_t p, uint64_t n, const uint64_t* __restrict__ pofs,
                                        const RdSpan* __restrict__ span) {
    uint64_t a = 1, b = n;                           // smallest j in [1, n] with pofs[j] > p (pofs[n] = P > p)
    while (a < b) {
        const uint64_t mid = (a + b) >> 1;
        if (pofs[mid] > p) b = mid; else a = mid + 1;
    }
    Piece pc;
    pc.rec = a - 1;
    pc.s = pofs[pc.rec];
    pc.e = pofs[a];
    pc.sp = span[pc.rec];
    const uint64_t k = p - pc.s;
    pc.line = (pc.sp.p & ~63ull) + (k << 6);
    const uint64_t end = pc.sp.p + pc.sp.len;
    pc.lo = pc.sp.p > pc.line ? (int)(pc.sp.p - pc.line) : 0;
    pc.hi = end < pc.line + 64 ? (int)(end - pc.line) : 64;
    pc.safe = (k != 0 || (pc.sp.flags & RD_SAFE_FIRST)) && (p + 1 != pc.e || (pc.sp.flags & RD_SAFE_LAST));
    return pc;
}

#define STEP4(reg, x, T) { const uint32_t x_ = (reg) ^ (x); \
    (reg) = T[768 + (x_ & 0xff)] ^ T[512 + ((x_ >> 8) & 0xff)] ^ T[256 + ((x_ >> 16) & 0xff)] ^ T[x_ >> 24]; }
#define STEP1(reg, byte, T) { (reg) = T[((reg) ^ (byte)) & 0xff] ^ ((reg) >> 8); }

template <int D>
__device__ __forceinline__ void seg_step(uint32_t& v, int lane, int first) {
    const bool take = lane - D >= first;             // (first >= 0: lane >= D as well)
    if (!__any(take)) return;                        // wave-uniform: no segment here reaches D lanes back
    const uint32_t t = __shfl_up(v, D, 64);
    if (take) v ^= mul_const<c_x8n(64ull * D)>(t);
}

__global__ __launch_bounds__(RD_NT) void k_rd_crc(uint64_t n, uint64_t P, const uint64_t* __restrict__ pofs,
                                                  const RdSpan* __restrict__ span, const uint32_t* __restrict__ tab,
                                                  int32_t* __restrict__ status, uint32_t* __restrict__ slot) {
    __shared__ uint32_t T[1024];
    for (int k = threadIdx.x; k < 1024; k += RD_NT) T[k] = tab[k];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t g0 = ((uint64_t)blockIdx.x * (RD_NT / 64) + (threadIdx.x >> 6)) * RD_IT;
    for (int it = 0; it < RD_IT; it++) {
        const uint64_t g = g0 + it, p0 = g << 6, p = p0 + lane;
        if (p0 >= P) return;                         // (wave-uniform)
        const bool act = p < P;
        uint32_t reg = 0;
        int first = lane;
        Piece pc;
        pc.rec = 0; pc.s = 0; pc.e = 0; pc.hi = 0; pc.lo = 0;
        if (act) {
            pc = locate(p, n, pofs, span);
            first = pc.s > p0 ? (int)(pc.s - p0) : 0;
            if (pc.safe) {
                const uint4* src = (const uint4*)pc.line;
                const uint4 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3];
                const uint32_t w[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                                        q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
                const int lo = pc.lo, hi = pc.hi;
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int b0 = 4 * k;
                    if (b0 < hi) {
                        uint32_t x = w[k];
                        // bytes below lo become zero: a zero register stays zero over them
                        if (lo > b0) x = (lo - b0 >= 4) ? 0u : x & (0xFFFFFFFFu << (8 * (lo - b0)));
                        if (hi - b0 >= 4) STEP4(reg, x, T)
                        else for (int j = 0; j < hi - b0; j++) STEP1(reg, x >> (8 * j), T)
                    }
                }
            } else {
                // a line that sticks out of the file: only the span's own bytes
                const uint8_t* src = (const uint8_t*)pc.line;
                for (int j = pc.lo; j < pc.hi; j++) STEP1(reg, (uint32_t)src[j], T)
            }
        }
        // segmented inclusive scan: v[j] = XOR over the record's lanes i <= j of A^(64 (j - i)) reg[i]
        uint32_t v = reg;
        seg_step<1>(v, lane, first);
        seg_step<2>(v, lane, first);
        seg_step<4>(v, lane, first);
        seg_step<8>(v, lane, first);
        seg_step<16>(v, lane, first);
        seg_step<32>(v, lane, first);
        uint32_t ex = __shfl_up(v, 1, 64);           // the lanes before this one, seen at this line's start
        if (lane == 0 || lane - 1 < first) ex = 0;
        if (!act) continue;
        const bool starts_here = pc.s >= p0;
        if (p + 1 == pc.e) {
            // the record's last piece: hi bytes from the line's start (a one-piece record has ex = 0)
            const uint32_t total = (ex ? cly_multmodp(tab[RT_X8 + pc.hi], ex) : 0u) ^ reg;
            if (starts_here) { if (total != pc.sp.want) status[pc.rec] = CLY_ERR_CRC; }
            else slot[2 * g] = total;                // entered from an earlier wave
        } else if (lane == 63) {
            slot[2 * g + (starts_here ? 1 : 0)] = v; // leaves the wave: everything up to this line's end
        }
    }
}

// One wave per multi-wave record: wave w of the record's piece range left
// its partial in slot[2w + 1] (the record's first wave) or slot[2w].
__global__ __launch_bounds__(64) void k_rd_finish(uint64_t n_multi, const uint64_t* __restrict__ multi,
                                                  const uint64_t* __restrict__ pofs, const RdSpan* __restrict__ span,
                                                  const uint32_t* __restrict__ slot, int32_t* __restrict__ status) {
    const uint64_t m = blockIdx.x;
    if (m >= n_multi) return;
    const uint64_t i = multi[m], s = pofs[i], e = pofs[i + 1];
    const RdSpan sp = span[i];
    const uint64_t w0 = s >> 6, w1 = (e - 1) >> 6, end = sp.p + sp.len, l0 = sp.p & ~63ull;
    uint32_t acc = 0;
    for (uint64_t w = w0 + threadIdx.x; w <= w1; w += 64) {
        const uint32_t r = w == w0 ? slot[2 * w + 1] : slot[2 * w];
        const uint64_t k1 = (e < ((w + 1) << 6) ? e : ((w + 1) << 6)) - s;      // the record's pieces up to this wave's end
        const uint64_t cov = l0 + (k1 << 6) < end ? l0 + (k1 << 6) : end;
        acc ^= cly_shift(r, end - cov);
    }
    for (int d = 32; d >= 1; d >>= 1) acc ^= __shfl_xor(acc, d, 64);
    if (threadIdx.x == 0 && acc != sp.want) status[i] = CLY_ERR_CRC;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// Final statuses -> value sizes (vs[n] = 0 closes the scan), the zero tuple of
// a failed CRC, the counters.
__global__ __launch_bounds__(RD_NT) void k_rd_vs(uint64_t n, const cly_pos* __restrict__ pos,
                                                 const int32_t* __restrict__ status, const RdSpan* __restrict__ span,
                                                 cly_tuple* __restrict__ tuples, uint64_t* __restrict__ vs,
                                                 RdTot* __restrict__ tot) {
    const uint64_t i = (uint64_t)blockIdx.x * RD_NT + threadIdx.x;
    unsigned long long c_rec = 0, c_eof = 0, c_crc = 0, c_oth = 0, c_nof = 0, vb = 0, rb = 0;
    if (i < n) {
        const int32_t st = status[i];
        if (st == CLY_READ_REC) {
            const RdSpan sp = span[i];
            c_rec = 1; vb = sp.len - sp.vrel; rb = sp.len + 4;
        } else if (st == CLY_READ_NOFILE) c_nof = 1;
        else if (st >= 0) c_eof = 1;
        else if (st == CLY_ERR_CRC) {
            c_crc = 1;
            if (tuples) {
                const cly_pos ps = pos[i];
                cly_tuple t;
                t.offset = ps.offset; t.expiration = 0; t.tx_id = 0; t.fid = ps.fid; t.size = 0; t.key_size = 0;
                t.value_size = 0; t.type = 0; t.data_type = 0; t.header_size = 0; t.txid_len = 0; t.crc = 0;
                tuples[i] = t;
            }
        } else c_oth = 1;
        vs[i] = vb;
    } else if (i == n) vs[n] = 0;
    c_rec = wave_sum(c_rec); c_eof = wave_sum(c_eof); c_crc = wave_sum(c_crc); c_oth = wave_sum(c_oth);
    c_nof = wave_sum(c_nof); vb = wave_sum(vb); rb = wave_sum(rb);
    if ((threadIdx.x & 63) == 0) {
        if (c_rec) atomicAdd(&tot->n_rec, c_rec);
        if (c_eof) atomicAdd(&tot->n_eof, c_eof);
        if (c_crc) atomicAdd(&tot->n_crc, c_crc);
        if (c_oth) atomicAdd(&tot->n_other, c_oth);
        if (c_nof) atomicAdd(&tot->n_nofile, c_nof);
        if (vb) atomicAdd(&tot->value_bytes, vb);
        if (rb) atomicAdd(&tot->record_bytes, rb);
    }
}

// The value part of every piece of a verified record -> values + val_off[rec].
// Source and destination alignments differ per record: bytes up to a dword
// boundary of the destination, then dwords, then the tail bytes.
__global__ __launch_bounds__(RD_NT) void k_rd_gather(uint64_t n, uint64_t P, const uint64_t* __restrict__ pofs,
                                                     const RdSpan* __restrict__ span,
                                                     const int32_t* __restrict__ status,
                                                     const uint64_t* __restrict__ val_off,
                                                     uint8_t* __restrict__ values) {
    const int lane = threadIdx.x & 63;
    const uint64_t g0 = ((uint64_t)blockIdx.x * (RD_NT / 64) + (threadIdx.x >> 6)) * RD_IT;
    for (int it = 0; it < RD_IT; it++) {
        const uint64_t p = ((g0 + it) << 6) + lane;
        if (p >= P) return;
        const Piece pc = locate(p, n, pofs, span);
        if (status[pc.rec] != CLY_READ_REC) continue;
        const uint64_t v0 = pc.sp.p + pc.sp.vrel;                    // the value's first byte
        uint64_t a = pc.line + pc.lo;
        const uint64_t b = pc.line + pc.hi;
        if (a < v0) a = v0;
        if (a >= b) continue;
        const uint8_t* src = (const uint8_t*)a;
        uint8_t* dst = values + val_off[pc.rec] + (a - v0);
        uint32_t m = (uint32_t)(b - a);
        while (m && ((uintptr_t)dst & 3)) { *dst++ = *src++; m--; }
        while (m >= 4) {
            uint32_t x;
            __builtin_memcpy(&x, src, 4);
            *(uint32_t*)dst = x;
            dst += 4; src += 4; m -= 4;
        }
        while (m) { *dst++ = *src++; m--; }
    }
}

// ---------------------------------------------------------------------------
// Host side
static const uint32_t* const_table() {
    static uint32_t t[RT_WORDS];
    static bool built = false;
    if (!built) {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ CLY_POLY : c >> 1;
            t[i] = c;
        }
        for (int k = 1; k < 4; k++)
            for (uint32_t i = 0; i < 256; i++) t[256 * k + i] = (t[256 * (k - 1) + i] >> 8) ^ t[t[256 * (k - 1) + i] & 0xff];
        for (uint32_t nb = 0; nb <= 64; nb++) t[RT_X8 + nb] = cly_x8n(nb);
        built = true;
    }
    return t;
}

// files sorted by fid; CLY_ERR_ARG for a duplicate fid, a null base of a
// non-empty file or a file of 2^47 bytes or more
static int sort_files(const cly_file* files, int nfiles, std::vector<RdFile>& out) {
    if (nfiles < 0 || (nfiles > 0 && !files)) return CLY_ERR_ARG;
    out.resize((size_t)nfiles);
    for (int i = 0; i < nfiles; i++) {
        if (files[i].len > RD_MAX_FILE_LEN || (files[i].len && !files[i].base)) return CLY_ERR_ARG;
        out[i].base = (uint64_t)(uintptr_t)files[i].base; out[i].len = files[i].len; out[i].fid = files[i].fid; out[i]._pad = (uint32_t)i;
    }
    std::sort(out.begin(), out.end(), [](const RdFile& a, const RdFile& b) { return a.fid < b.fid; });
    for (int i = 1; i < nfiles; i++) if (out[i].fid == out[i - 1].fid) return CLY_ERR_ARG;
    return CLY_OK;
}

// The device pipeline.  own_values: the host entry's mode, where the value
// buffer is taken from the context's scratch once the need is known
// (*own_values receives it; values_cap is still the caller's limit).
static int read_impl(cly_ctx* ctx, const std::vector<RdFile>& sorted, const cly_pos* d_pos, uint64_t n,
                     cly_tuple* d_tuples, int32_t* d_status, uint64_t* d_val_off, uint8_t* d_values,
                     uint64_t values_cap, uint8_t** own_values, cly_read_result* rr, hipStream_t st) {
    int rc = CLY_OK;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const int nfiles = (int)sorted.size();
    const bool want_values = d_values != nullptr || own_values != nullptr;
    uint32_t* d_tab; RdFile* d_files; RdSpan* d_span; uint64_t* d_cnt; uint64_t* d_pofs; uint64_t* d_multi;
    RdTot* d_tot; uint32_t* d_slot; void* d_tmp;
    size_t tmp_bytes = 0;
    RdTot tot;
    uint64_t P = 0;
    memset(rr, 0, sizeof(*rr));
    if (hipSetDevice(ctx->device) != hipSuccess) return CLY_ERR_DEVICE;
    if (n == 0) {
        CLY_CKG(hipMemsetAsync(d_val_off, 0, sizeof(uint64_t), st));
        CLY_CKG(hipStreamSynchronize(st));
        return CLY_OK;
    }
    CLY_CKG(hipEventCreateWithFlags(&e0, hipEventDisableSystemFence));      // (timing only)
    CLY_CKG(hipEventCreateWithFlags(&e1, hipEventDisableSystemFence));
    CLY_CKG(cly_scratch(ctx, RS_TAB, sizeof(uint32_t) * RT_WORDS, &d_tab));
    CLY_CKG(cly_scratch(ctx, RS_FILES, sizeof(RdFile) * (size_t)nfiles, &d_files));
    CLY_CKG(cly_scratch(ctx, RS_SPAN, sizeof(RdSpan) * n, &d_span));
    CLY_CKG(cly_scratch(ctx, RS_CNT, sizeof(uint64_t) * (n + 1), &d_cnt));
    CLY_CKG(cly_scratch(ctx, RS_POFS, sizeof(uint64_t) * (n + 1), &d_pofs));
    CLY_CKG(cly_scratch(ctx, RS_MULTI, sizeof(uint64_t) * n, &d_multi));
    CLY_CKG(cly_scratch(ctx, RS_TOT, sizeof(RdTot), &d_tot));
    CLY_CKG(rocprim::exclusive_scan(nullptr, tmp_bytes, d_cnt, d_pofs, (uint64_t)0, (size_t)(n + 1),
                                    rocprim::plus<uint64_t>(), st));
    CLY_CKG(cly_scratch(ctx, RS_TMP, tmp_bytes, &d_tmp));
    CLY_CKG(hipMemcpyAsync(d_tab, const_table(), sizeof(uint32_t) * RT_WORDS, hipMemcpyHostToDevice, st));
    if (nfiles) CLY_CKG(hipMemcpyAsync(d_files, sorted.data(), sizeof(RdFile) * (size_t)nfiles, hipMemcpyHostToDevice, st));
    CLY_CKG(hipEventRecord(e0, st));
    CLY_CKG(hipMemsetAsync(d_tot, 0, sizeof(RdTot), st));
    {
        const unsigned grid = (unsigned)((n + 1 + RD_NT - 1) / RD_NT);
        k_rd_hdr<<<grid, RD_NT, 0, st>>>(n, d_pos, d_files, nfiles, d_tuples, d_status, d_span, d_cnt);
        CLY_CKG(hipGetLastError());
        size_t tb = tmp_bytes;
        CLY_CKG(rocprim::exclusive_scan(d_tmp, tb, d_cnt, d_pofs, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st));
        k_rd_plan<<<grid, RD_NT, 0, st>>>(n, d_pofs, d_multi, d_tot);
        CLY_CKG(hipGetLastError());
        // the sizes of the hot pass: one small read-back
        CLY_CKG(hipMemcpyAsync(&P, d_pofs + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        CLY_CKG(hipMemcpyAsync(&tot, d_tot, sizeof(RdTot), hipMemcpyDeviceToHost, st));
        CLY_CKG(hipStreamSynchronize(st));
        const uint64_t ngroups = (P + 63) >> 6;
        const unsigned pgrid = (unsigned)((ngroups + (RD_NT / 64) * RD_IT - 1) / ((RD_NT / 64) * RD_IT));
        if (P) {
            CLY_CKG(cly_scratch(ctx, RS_SLOT, sizeof(uint32_t) * 2 * ngroups, &d_slot));
            k_rd_crc<<<pgrid, RD_NT, 0, st>>>(n, P, d_pofs, d_span, d_tab, d_status, d_slot);
            CLY_CKG(hipGetLastError());
            if (tot.n_multi) {
                k_rd_finish<<<(unsigned)tot.n_multi, 64, 0, st>>>(tot.n_multi, d_multi, d_pofs, d_span, d_slot, d_status);
                CLY_CKG(hipGetLastError());
            }
        }
        k_rd_vs<<<grid, RD_NT, 0, st>>>(n, d_pos, d_status, d_span, d_tuples, d_cnt, d_tot);
        CLY_CKG(hipGetLastError());
        tb = tmp_bytes;
        CLY_CKG(rocprim::exclusive_scan(d_tmp, tb, d_cnt, d_val_off, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st));
        CLY_CKG(hipMemcpyAsync(&tot, d_tot, sizeof(RdTot), hipMemcpyDeviceToHost, st));
        CLY_CKG(hipStreamSynchronize(st));
        rr->n_rec = tot.n_rec; rr->n_eof = tot.n_eof; rr->n_crc = tot.n_crc; rr->n_other = tot.n_other;
        rr->n_nofile = tot.n_nofile; rr->value_bytes = tot.value_bytes; rr->record_bytes = tot.record_bytes;
        if (want_values && tot.value_bytes > values_cap) rc = CLY_ERR_CAPACITY;
        else if (want_values && tot.value_bytes && P) {
            if (own_values) {
                CLY_CKG(cly_scratch(ctx, RS_H_VAL, tot.value_bytes, &d_values));
                *own_values = d_values;
            }
            k_rd_gather<<<pgrid, RD_NT, 0, st>>>(n, P, d_pofs, d_span, d_status, d_val_off, d_values);
            CLY_CKG(hipGetLastError());
        }
    }
    CLY_CKG(hipEventRecord(e1, st));
    CLY_CKG(hipEventSynchronize(e1));
    {
        float ms = 0;
        CLY_CKG(hipEventElapsedTime(&ms, e0, e1));
        rr->read_ms = ms;
    }
done:
    if (rc == CLY_ERR_DEVICE) hipStreamSynchronize(st);           // (the buffers stay in the context's scratch)
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    return rc;
}

extern "C" int cly_read_device(cly_ctx* ctx, const cly_file* files, int nfiles, const cly_pos* d_pos, uint64_t n,
                               cly_tuple* d_tuples, int32_t* d_status, uint64_t* d_val_off, uint8_t* d_values,
                               uint64_t values_cap, cly_read_result* rr, void* stream) {
    if (!ctx || !rr || !d_status || !d_val_off || (n > 0 && !d_pos)) return CLY_ERR_ARG;
    std::vector<RdFile> sorted;
    const int rc = sort_files(files, nfiles, sorted);
    if (rc != CLY_OK) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    return read_impl(ctx, sorted, d_pos, n, d_tuples, d_status, d_val_off, d_values, values_cap, nullptr, rr, st);
}

extern "C" int cly_read(cly_ctx* ctx, const cly_file* files, int nfiles, const cly_pos* pos, uint64_t n,
                        cly_tuple* tuples, int32_t* status, uint64_t* val_off, uint8_t* values, uint64_t values_cap,
                        cly_read_result* rr) {
    if (!ctx || !rr || !status || !val_off || (n > 0 && !pos)) return CLY_ERR_ARG;
    std::vector<RdFile> sorted;
    int rc = sort_files(files, nfiles, sorted);
    if (rc != CLY_OK) return rc;
    if (hipSetDevice(ctx->device) != hipSuccess) return CLY_ERR_DEVICE;
    hipStream_t st = ctx->stream;
    // stage only the files that a position names
    std::vector<uint8_t> named((size_t)nfiles, 0);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t fid = pos[i].fid;
        auto it = std::lower_bound(sorted.begin(), sorted.end(), fid, [](const RdFile& f, uint32_t v) { return f.fid < v; });
        if (it != sorted.end() && it->fid == fid) named[(size_t)(it - sorted.begin())] = 1;
    }
    std::vector<RdFile> dev;
    uint64_t bytes = 0;
    for (int i = 0; i < nfiles; i++) if (named[i]) { dev.push_back(sorted[i]); bytes += (sorted[i].len + 255) & ~255ull; }
    uint8_t* d_bytes = nullptr; cly_pos* d_pos = nullptr; cly_tuple* d_tup = nullptr; int32_t* d_status = nullptr;
    uint64_t* d_voff = nullptr; uint8_t* d_val = nullptr;
    CLY_CKG(cly_scratch(ctx, RS_H_BYTES, bytes, &d_bytes));
    CLY_CKG(cly_scratch(ctx, RS_H_POS, sizeof(cly_pos) * n, &d_pos));
    if (tuples) CLY_CKG(cly_scratch(ctx, RS_H_TUP, sizeof(cly_tuple) * n, &d_tup));
    CLY_CKG(cly_scratch(ctx, RS_H_STATUS, sizeof(int32_t) * n, &d_status));
    CLY_CKG(cly_scratch(ctx, RS_H_VOFF, sizeof(uint64_t) * (n + 1), &d_voff));
    {
        uint64_t at = 0;
        for (RdFile& f : dev) {
            if (f.len) CLY_CKG(hipMemcpyAsync(d_bytes + at, (const void*)(uintptr_t)f.base, f.len, hipMemcpyHostToDevice, st));
            f.base = (uint64_t)(uintptr_t)(d_bytes + at);
            at += (f.len + 255) & ~255ull;
        }
    }
    if (n) CLY_CKG(hipMemcpyAsync(d_pos, pos, sizeof(cly_pos) * n, hipMemcpyHostToDevice, st));
    rc = read_impl(ctx, dev, d_pos, n, d_tup, d_status, d_voff, nullptr, values ? values_cap : 0,
                   values ? &d_val : nullptr, rr, st);
    if (rc == CLY_OK || rc == CLY_ERR_CAPACITY) {
        const int rc0 = rc;
        if (n && tuples) CLY_CKG(hipMemcpyAsync(tuples, d_tup, sizeof(cly_tuple) * n, hipMemcpyDeviceToHost, st));
        if (n) CLY_CKG(hipMemcpyAsync(status, d_status, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        CLY_CKG(hipMemcpyAsync(val_off, d_voff, sizeof(uint64_t) * (n + 1), hipMemcpyDeviceToHost, st));
        if (rc0 == CLY_OK && d_val && rr->value_bytes)
            CLY_CKG(hipMemcpyAsync(values, d_val, rr->value_bytes, hipMemcpyDeviceToHost, st));
        CLY_CKG(hipStreamSynchronize(st));
    }
done:
    return rc;
}

// The serial form this entry replaces, for tools/read_bench.py's floor (not in
// the public header): cly_db_value's loop over host memory on the calling
// thread: step_hdr, a byte-wise table CRC, a memcpy of the value.  Returns
// the records read; *value_bytes / *record_bytes as cly_read_result's.
extern "C" uint64_t cly_dbg_read_host(const uint8_t* base, uint64_t len, const cly_pos* pos, uint64_t n,
                                      uint8_t* values, uint64_t cap, uint64_t* value_bytes, uint64_t* record_bytes) {
    const uint32_t* T = const_table();
    uint64_t nrec = 0, vb = 0, rb = 0;
    for (uint64_t i = 0; i < n; i++) {
        const int64_t off = pos[i].offset;
        if (off < 0) continue;
        const Hdr h = step_hdr(base, off, (int64_t)len, off);
        if (h.status != REC_OK) continue;
        uint32_t c = 0xFFFFFFFFu;
        const uint8_t* p = base + off + 4;
        for (int64_t k = 0; k < h.size - 4; k++) c = T[(c ^ p[k]) & 0xff] ^ (c >> 8);
        if (~c != h.crc) continue;
        if (values && vb + h.vs <= cap) memcpy(values + vb, base + off + h.hsz + h.ks, h.vs);
        nrec++; vb += h.vs; rb += (uint64_t)h.size;
    }
    if (value_bytes) *value_bytes = vb;
    if (record_bytes) *record_bytes = rb;
    return nrec;
}
