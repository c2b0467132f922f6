// clymerge.hip — db.merge's rewrite loop on the device (gfx950), part of
// libclyscan.so (C-ABI: cly_merge_device / cly_merge in include/clyscan.h).
//
// Reference (merge.go:90-143): for every record the scan of the old files
// returns, in file order, look the realKey up in the index; when the index
// still points at (fid, offset) the record is live and is re-appended to the
// merge DB with Key = encodeKeyWithTxId(realKey, NO_TX_ID) (batch.go:120-127)
// through appendLogRecord (db.go:368-413: EncodeLogRecord, a new file when
// WriteOff+size > DataFileSize), and a hint record {realKey,
// EncodeLogRecordPos(pos)} (data/dataFile.go:114-121, data/logRecord.go:117-124)
// is written to the hint-index file.  The index lookup itself is the
// caller's: it arrives as one live byte per scanned tuple.
//
// Device pipeline (one stream):
//   k_mplan     per tuple: new record size (0 when dead), verbatim or re-encoded; block sums
//   k_msums     exclusive scan of the block sums (one workgroup)
//   k_mcompact  live records compacted in order: pre-rotation byte offset g
//   k_mrot      appendLogRecord's rotation: first record of every output file
//               (1024-ary searches over g, one workgroup)
//   k_mplace    per live record: output file/offset, copy descriptor, 4-KiB
//               block map, re-encoded header + CRC, hint record size
//   k_msums, k_mhint   hint record offsets, hint records (header, realKey, pos, CRC)
//   k_mcopy     output files by 4-KiB destination blocks: 16-B stores,
//               funnel-shifted dword loads of the source
// A live record whose key already is 0x00||realKey and whose header is the
// canonical encoding (every non-transactional record the writer produces) is
// byte-identical after EncodeLogRecord: it is copied as is, CRC included.
// Other live records get a new header; their CRC is the stored one corrected
// by the header+key difference, shifted over the value
// (crc' = crc ^ A^(8 vs) (R(~0, X_old) ^ R(~0, X_new))), so the value bytes are
// read only once, by the copy.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "scan_core.h"

#define CLY_TAG "clymerge"
#include "cly_internal.h"

#define M_NT 256
#define M_IT 16
#define M_BLK (M_NT * M_IT)          // tuples (or live records) per workgroup of the scans
#define MP_FILES 512                 // input / output files whose bounds k_mplace keeps in LDS
#define M_PRE 32                     // bytes per re-encoded prefix (crc..header, 0x00): <= 27
#define M_CB 4096                    // destination block of k_mcopy
#define M_CMAX 512                   // records starting in one block (>= M_CB / 10 + 2)
#define PLAN_RE (1ull << 32)         // plan bit: re-encoded
// k_mplan -> k_mcompact -> k_mplace, per live record: file offset (bits 0-31),
// header + txId bytes (32-39), realKey length (40-55); PK_SLOW: read the tuple
#define PK_SLOW (1ull << 56)

struct MSum { unsigned long long bytes, count; };
struct MEnt { uint64_t g; uint32_t tuple, nsz; };
// pre: the re-encoded prefix's bytes (bits 0-7; 0: verbatim from src); for
// the merge also the realKey's offset from src (bits 8-15) and its length
// (bits 16-31, 0xFFFF: longer), for the hint records
struct MCopy { uint64_t dst, src; uint32_t size, pre; };
#define MC_PRE(x) ((x) & 0xFFu)
#define MC_KOFF(x) (((x) >> 8) & 0xFFu)
#define MC_RK(x) ((x) >> 16)
#define MH_KEY 16                    // realKey bytes k_mcopy keeps per live record for k_mhint
struct MTot {                        // device totals, read back by the host
    unsigned long long nl, bytes, hint_bytes, n_re;
    uint32_t n_out, bad;
};

__device__ __forceinline__ uint64_t zz(int64_t x) {
    const uint64_t u = (uint64_t)x << 1;
    return x < 0 ? ~u : u;
}
__device__ __forceinline__ int uvlen(uint64_t u) {
    int n = 1;
    while (u >= 0x80) { u >>= 7; n++; }
    return n;
}
__device__ __forceinline__ int put_uv(uint8_t* b, uint64_t u) {
    int n = 0;
    while (u >= 0x80) { b[n++] = (uint8_t)(u | 0x80); u >>= 7; }
    b[n++] = (uint8_t)u;
    return n;
}
__device__ __forceinline__ int find_file_u64(const uint64_t* first, int nfiles, uint64_t i) {
    int lo = 0, hi = nfiles - 1;                      // largest f with first[f] <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ void crc_table_init(uint32_t* t) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        uint32_t s = (uint32_t)i;
        for (int k = 0; k < 8; k++) s = (s & 1) ? (s >> 1) ^ CLY_POLY : s >> 1;
        t[i] = s;
    }
    __syncthreads();
}
__device__ __forceinline__ uint32_t crc_upd(const uint32_t* t, uint32_t s, uint32_t b) {
    return t[(s ^ b) & 0xff] ^ (s >> 8);
}
// slicing-by-4 tables t4[k*256 + v] = A^(8k) T0[v] (t4[0..255] = T0)
__device__ __forceinline__ void crc_table4_init(uint32_t* t4) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        uint32_t s = (uint32_t)i;
        for (int k = 0; k < 8; k++) s = (s & 1) ? (s >> 1) ^ CLY_POLY : s >> 1;
        t4[i] = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        uint32_t s = t4[i];
        for (int k = 1; k < 4; k++) { s = t4[s & 0xff] ^ (s >> 8); t4[k * 256 + i] = s; }
    }
    __syncthreads();
}
// register over len bytes at p (any alignment): bytes up to a dword boundary,
// then aligned dwords four at a time (loads in flight together), then the tail
__device__ __forceinline__ uint32_t crc_span(const uint32_t* t4, uint32_t s, const uint8_t* p, uint64_t len) {
    while (len && ((uintptr_t)p & 3)) { s = crc_upd(t4, s, *p++); len--; }
    const uint32_t* w = (const uint32_t*)p;
    uint64_t nw = len >> 2;
    while (nw >= 16) {                          // 16 independent loads in flight, then the steps
        uint32_t v[16];
        #pragma unroll
        for (int k = 0; k < 16; k++) v[k] = w[k];
        #pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint32_t x = s ^ v[k];
            s = t4[768 + (x & 0xff)] ^ t4[512 + ((x >> 8) & 0xff)] ^ t4[256 + ((x >> 16) & 0xff)] ^ t4[x >> 24];
        }
        w += 16;
        nw -= 16;
    }
    while (nw >= 4) {
        const uint32_t a = w[0], b = w[1], c = w[2], d = w[3];
        #pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t x = s ^ (k == 0 ? a : k == 1 ? b : k == 2 ? c : d);
            s = t4[768 + (x & 0xff)] ^ t4[512 + ((x >> 8) & 0xff)] ^ t4[256 + ((x >> 16) & 0xff)] ^ t4[x >> 24];
        }
        w += 4;
        nw -= 4;
    }
    while (nw) {
        const uint32_t x = s ^ *w++;
        s = t4[768 + (x & 0xff)] ^ t4[512 + ((x >> 8) & 0xff)] ^ t4[256 + ((x >> 16) & 0xff)] ^ t4[x >> 24];
        nw--;
    }
    p = (const uint8_t*)w;
    for (uint64_t q = 0; q < (len & 3); q++) s = crc_upd(t4, s, p[q]);
    return s;
}

// Block-wide exclusive scan of (a, b) pairs over M_NT threads.
__device__ __forceinline__ MSum block_excl(MSum v, MSum& total, MSum* sh) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    MSum inc = v;
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long a = __shfl_up(inc.bytes, d, 64), c = __shfl_up(inc.count, d, 64);
        if (lane >= d) { inc.bytes += a; inc.count += c; }
    }
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    MSum base = {0, 0};
    total.bytes = 0; total.count = 0;
    for (int k = 0; k < M_NT / 64; k++) {
        if (k < w) { base.bytes += sh[k].bytes; base.count += sh[k].count; }
        total.bytes += sh[k].bytes; total.count += sh[k].count;
    }
    __syncthreads();
    MSum ex = {base.bytes + inc.bytes - v.bytes, base.count + inc.count - v.count};
    return ex;
}

// ---- k_mplan: per tuple, the size of its merge record (0 = dead) ----------
// Canonical check: EncodeLogRecord writes PutVarint(len(key)), PutVarint(len(value)),
// PutVarint(exp) (data/logRecord.go:66-68); a record is kept byte for byte iff its
// key already is varint(0)||realKey and its stored header bytes are that encoding.
__global__ void __launch_bounds__(M_NT)
k_mplan(const cly_tuple* __restrict__ tup, uint64_t T, const uint8_t* __restrict__ live,
        const uint64_t* __restrict__ first, const uint64_t* __restrict__ bases, int nfiles,
        uint64_t* plan, uint64_t* pk, MSum* bsum, uint64_t dfs, MTot* tot) {
    __shared__ MSum sh[M_NT / 64];
    MSum acc = {0, 0};
    const uint64_t b0 = (uint64_t)blockIdx.x * M_BLK;
    for (int k = 0; k < M_IT; k++) {
        const uint64_t i = b0 + (uint64_t)k * M_NT + threadIdx.x;
        if (i >= T) break;
        uint64_t p = 0, pkv = 0;               // (every slot written: whole lines)
        if (live[i] == 1) {                 // CLY_IX_LIVE; a CLY_IX_HOST byte is not a verdict
            const cly_tuple t = tup[i];
            if (t.txid_len == 0xFF) { atomicOr(&tot->bad, 1u); plan[i] = 0; pk[i] = 0; continue; }   // parseLogRecordKey panics
            const uint32_t rk = t.key_size - t.txid_len;
            const uint64_t nks = (uint64_t)rk + 1;
            const int nh = 6 + uvlen(zz((int64_t)nks)) + uvlen(zz((int64_t)t.value_size)) + uvlen(zz(t.expiration));
            const uint64_t nsz = (uint64_t)nh + nks + t.value_size;
            bool verbatim = t.txid_len == 1 && t.tx_id == 0 && nh == t.header_size;
            // Equal header lengths mean the stored varints are the canonical ones
            // (a longer-than-canonical encoding would make the header longer) unless
            // a stored size varint was truncated by uint32() (data/logRecord.go:101,106),
            // which needs >= 5 varint bytes: only then compare the bytes.
            if (verbatim && (uvlen(zz((int64_t)nks)) >= 5 || uvlen(zz((int64_t)t.value_size)) >= 5)) {
                const int f = find_file_u64(first, nfiles, i);
                const uint8_t* h = (const uint8_t*)bases[f] + t.offset;
                uint8_t cb[26];
                int n = 6;
                n += put_uv(cb + n, zz((int64_t)nks));
                n += put_uv(cb + n, zz((int64_t)t.value_size));
                n += put_uv(cb + n, zz(t.expiration));
                for (int q = 6; q < n && verbatim; q++) verbatim = h[q] == cb[q];
            }
            if (nsz > dfs) atomicOr(&tot->bad, 2u);              // one record per file would not fit
            p = nsz | (verbatim ? 0ull : PLAN_RE);
            // what k_mplace needs of a copied record, so that it reads no tuple
            const uint32_t hx = (uint32_t)t.header_size + t.txid_len;
            const bool esc = !verbatim || rk >= 0xFFFFu || hx > 0xFFu || (uint64_t)t.offset >= (1ull << 32);
            pkv = esc ? PK_SLOW : (uint64_t)t.offset | ((uint64_t)hx << 32) | ((uint64_t)rk << 40);
            acc.bytes += nsz;
            acc.count += 1;
        }
        plan[i] = p;
        pk[i] = pkv;
    }
    // block sum (order-free)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        acc.bytes += __shfl_xor(acc.bytes, d, 64);
        acc.count += __shfl_xor(acc.count, d, 64);
    }
    if (lane == 0) sh[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        MSum s = {0, 0};
        for (int k = 0; k < M_NT / 64; k++) { s.bytes += sh[k].bytes; s.count += sh[k].count; }
        bsum[blockIdx.x] = s;
    }
}

// ---- k_msums: exclusive scan of block sums (one workgroup of M_NT threads) --
__global__ void __launch_bounds__(M_NT)
k_msums(MSum* bsum, uint64_t nblk, unsigned long long* out_bytes, unsigned long long* out_count) {
    __shared__ MSum sh[M_NT / 64];
    MSum carry = {0, 0};
    for (uint64_t b = 0; b < nblk; b += M_NT) {
        const uint64_t i = b + threadIdx.x;
        MSum v = i < nblk ? bsum[i] : MSum{0, 0};
        MSum total;
        MSum ex = block_excl(v, total, sh);
        if (i < nblk) bsum[i] = MSum{carry.bytes + ex.bytes, carry.count + ex.count};
        carry.bytes += total.bytes;
        carry.count += total.count;
    }
    if (threadIdx.x == 0) {
        if (out_bytes) *out_bytes = carry.bytes;
        if (out_count) *out_count = carry.count;
    }
}

// ---- k_mcompact: live records in order, with their pre-rotation offset -----
__global__ void __launch_bounds__(M_NT)
k_mcompact(const uint64_t* __restrict__ plan, const uint64_t* __restrict__ pk, uint64_t T,
           const MSum* __restrict__ bsum, MEnt* ent, uint64_t* pkc) {
    __shared__ MSum sh[M_NT / 64];
    const uint64_t b0 = (uint64_t)blockIdx.x * M_BLK;
    MSum carry = bsum[blockIdx.x];
    for (int k = 0; k < M_IT; k++) {
        const uint64_t i = b0 + (uint64_t)k * M_NT + threadIdx.x;
        if (b0 + (uint64_t)k * M_NT >= T) break;                 // (uniform)
        const uint64_t p = i < T ? plan[i] : 0;
        const uint32_t nsz = (uint32_t)p;
        MSum v = {nsz, nsz ? 1ull : 0ull};
        MSum total;
        const MSum ex = block_excl(v, total, sh);
        if (nsz) {
            ent[carry.count + ex.count] = MEnt{carry.bytes + ex.bytes, (uint32_t)i, nsz};
            pkc[carry.count + ex.count] = pk[i];
        }
        carry.bytes += total.bytes;
        carry.count += total.count;
    }
}

// ---- k_mrot: appendLogRecord's file rotation (db.go:376-385) ----------------
// File k starts at live record r_k; it holds r_k .. m-1 for the largest m with
// g(m) - g(r_k) <= DataFileSize (g(nl) = total bytes), at least one record.
// One workgroup; each search step probes M_ROT positions of the interval.
#define M_ROT 1024
__device__ __forceinline__ uint64_t g_at(const MEnt* e, uint64_t nl, uint64_t total, uint64_t m) {
    return m < nl ? e[m].g : total;
}
__global__ void __launch_bounds__(M_ROT)
k_mrot(const MEnt* __restrict__ e, MTot* tot, uint64_t dfs, uint32_t max_files, uint64_t* fstart, uint64_t* flen) {
    const uint64_t nl = tot->nl, total = tot->bytes;
    const uint64_t mean = nl ? (total / nl > 0 ? total / nl : 1) : 1;   // bytes per merge record
    __shared__ uint64_t s_lo, s_hi;
    uint64_t r = 0;
    uint32_t k = 0;
    while (r < nl) {
        const uint64_t g0 = e[r].g, lim = g0 + dfs;
        uint64_t lo = r + 1;                                    // g(r+1) - g(r) = size <= dfs (k_mplan)
        uint64_t hi = r + dfs / 10 + 2;                         // merge records are >= 10 bytes
        if (hi > nl) hi = nl;
        if (hi < lo) hi = lo;
        // first round: M_ROT consecutive positions around the end the mean
        // record size predicts (one round when the end is among them); then
        // evenly spread probes
        uint64_t guess = r + dfs / mean;
        bool first = true;
        while (lo < hi) {                                       // invariant: g(lo) <= lim
            const uint64_t span = hi - lo;
            uint64_t pos = lo + (span * (threadIdx.x + 1) + M_ROT - 1) / M_ROT;   // in (lo, hi]
            if (first) {
                const uint64_t q = guess + threadIdx.x;         // guess - M_ROT/2 .. guess + M_ROT/2 - 1, clamped
                pos = q < lo + 1 + M_ROT / 2 ? lo + 1 : q - M_ROT / 2;
                if (pos > hi) pos = hi;
                first = false;
            }
            const int ok = g_at(e, nl, total, pos) <= lim;
            const int c = __syncthreads_count(ok);              // monotone: probes 0..c-1 are ok
            if (threadIdx.x == (unsigned)c - 1) s_lo = pos;
            if (threadIdx.x == (unsigned)c) s_hi = pos - 1;
            if (threadIdx.x == 0) { if (c == 0) s_lo = lo; if (c == M_ROT) s_hi = hi; }
            __syncthreads();
            lo = s_lo; hi = s_hi;
            __syncthreads();
        }
        if (threadIdx.x == 0 && k < max_files) {
            fstart[k] = r;
            flen[k] = g_at(e, nl, total, lo) - g0;
        }
        r = lo;
        k++;
    }
    if (threadIdx.x == 0) {
        if (k < max_files) fstart[k] = nl;
        tot->n_out = k;
    }
}

// ---- k_mplace: per live record, where it goes --------------------------------
__global__ void __launch_bounds__(M_NT)
k_mplace(const MEnt* __restrict__ e, const uint64_t* __restrict__ pkc, const cly_tuple* __restrict__ tup,
         const uint64_t* __restrict__ plan,
         const uint64_t* __restrict__ first, const uint64_t* __restrict__ bases, int nfiles,
         const uint64_t* __restrict__ fstart, MTot* tot, uint64_t stride, MCopy* cp, uint8_t* pre,
         uint32_t* bmap, uint32_t* hsz, MSum* bsum) {
    __shared__ uint32_t tab[256];
    __shared__ MSum sh[M_NT / 64];
    // the two searches per record (input file of its tuple, output file of the
    // record) and the output files' first offsets, from LDS when they fit
    __shared__ uint64_t s_first[MP_FILES], s_fst[MP_FILES], s_fg[MP_FILES];
    crc_table_init(tab);
    const uint64_t nl = tot->nl;
    const uint32_t nout = tot->n_out;
    const bool lds_in = nfiles <= MP_FILES, lds_out = nout <= MP_FILES;
    if (lds_in) for (int i = threadIdx.x; i < nfiles; i += M_NT) s_first[i] = first[i];
    if (lds_out) for (uint32_t i = threadIdx.x; i < nout; i += M_NT) { s_fst[i] = fstart[i]; s_fg[i] = e[fstart[i]].g; }
    __syncthreads();
    MSum acc = {0, 0};
    unsigned long long nre = 0;
    const uint64_t b0 = (uint64_t)blockIdx.x * M_BLK;
    for (int it = 0; it < M_IT; it++) {
        const uint64_t j = b0 + (uint64_t)it * M_NT + threadIdx.x;
        if (j >= nl) break;
        const MEnt m = e[j];
        // output file: largest k with fstart[k] <= j
        int lo = 0, hi = (int)nout - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((lds_out ? s_fst[mid] : fstart[mid]) <= j) lo = mid; else hi = mid - 1;
        }
        const uint64_t off = m.g - (lds_out ? s_fg[lo] : e[fstart[lo]].g);
        const uint64_t dst = (uint64_t)lo * stride + off;
        const int f = find_file_u64(lds_in ? s_first : first, nfiles, m.tuple);
        const uint64_t q = pkc[j];
        MCopy c;
        c.dst = dst;
        c.size = m.nsz;
        uint32_t rk;
        if (!(q & PK_SLOW)) {
            // a record copied byte for byte: its file offset and header sizes
            // from k_mplan (no tuple read)
            rk = (uint32_t)(q >> 40) & 0xFFFFu;
            c.src = bases[f] + (uint32_t)q;
            c.pre = (rk << 16) | ((uint32_t)((q >> 32) & 0xFFu) << 8);
        } else {
        const cly_tuple t = tup[m.tuple];
        const uint8_t* F = (const uint8_t*)bases[f] + t.offset;
        rk = t.key_size - t.txid_len;
        const uint32_t kx = (rk < 0xFFFFu ? rk : 0xFFFFu) << 16;
        if (!(plan[m.tuple] & PLAN_RE)) {
            c.src = (uint64_t)F;
            c.pre = kx | ((uint32_t)(t.header_size + t.txid_len) << 8);
        } else {
            // new header: crc, type, dtype, varint(1+rk), varint(vs), varint(exp), then key byte 0x00
            uint8_t h[M_PRE];
            h[4] = t.type;
            h[5] = t.data_type;
            int n = 6;
            n += put_uv(h + n, zz((int64_t)rk + 1));
            n += put_uv(h + n, zz((int64_t)t.value_size));
            n += put_uv(h + n, zz(t.expiration));
            h[n] = 0x00;
            const uint8_t* rkey = F + t.header_size + t.txid_len;
            uint32_t ro = 0xFFFFFFFFu, rn = 0xFFFFFFFFu;
            for (uint32_t q = 4; q < (uint32_t)t.header_size + t.key_size; q++) ro = crc_upd(tab, ro, F[q]);
            for (int q = 4; q <= n; q++) rn = crc_upd(tab, rn, h[q]);
            for (uint32_t q = 0; q < rk; q++) rn = crc_upd(tab, rn, rkey[q]);
            const uint32_t crc = t.crc ^ cly_shift(ro ^ rn, t.value_size);
            h[0] = (uint8_t)crc; h[1] = (uint8_t)(crc >> 8); h[2] = (uint8_t)(crc >> 16); h[3] = (uint8_t)(crc >> 24);
            uint8_t* pj = pre + j * M_PRE;
            for (int q = 0; q <= n; q++) pj[q] = h[q];
            c.pre = kx | ((uint32_t)n + 1);
            c.src = (uint64_t)rkey;
            nre++;
        }
        }
        cp[j] = c;
        // blocks of k_mcopy whose first byte lies in this record
        for (uint64_t b = (dst + M_CB - 1) / M_CB; b * M_CB < dst + c.size; b++) bmap[b] = (uint32_t)j;
        // hint record: Key realKey, Value varint(fid)||varint(off), Type 0, DataType 0, Expiration 0
        const int plen = uvlen(zz((int64_t)lo)) + uvlen(zz((int64_t)off));
        const uint32_t hs = 6 + uvlen(zz((int64_t)rk)) + uvlen(zz((int64_t)plen)) + 1 + rk + plen;
        hsz[j] = hs;
        acc.bytes += hs;
        acc.count += 1;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        acc.bytes += __shfl_xor(acc.bytes, d, 64);
        acc.count += __shfl_xor(acc.count, d, 64);
        nre += __shfl_xor(nre, d, 64);
    }
    if (lane == 0 && nre) atomicAdd(&tot->n_re, nre);
    if (lane == 0) sh[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        MSum s = {0, 0};
        for (int k = 0; k < M_NT / 64; k++) { s.bytes += sh[k].bytes; s.count += sh[k].count; }
        bsum[blockIdx.x] = s;
    }
}

// ---- k_mhint: hint-index records (data/dataFile.go:114-121) -----------------
// Record of live record j: crc(4) 0 0 varint(rk) varint(pl) 0x00 realKey pos,
// pos = varint(fid) varint(off) (EncodeLogRecordPos), CRC over bytes 4 .. end.
// The records of a workgroup's 256 consecutive live records are contiguous in
// the hint file: each thread writes its bytes into an LDS stage laid out at
// the output's 16-B phase (header and pos from registers, realKey from aligned
// dword loads), then computes its CRC slicing-by-4 from the stage, and the
// workgroup stores the stage with 16-B stores.  A workgroup whose records
// exceed the stage (large keys) writes to global directly, CRC byte by byte.
#define MH_BUF 12288
#define CLY_GLB __attribute__((address_space(1)))            // global (not flat) loads
// Go's PutUvarint of u (< 2^56) packed little-endian, *n bytes
__device__ __forceinline__ uint64_t uv_pack(uint64_t u, int& n) {
    uint64_t r = 0;
    int k = 0;
    while (u >= 0x80) { r |= ((u & 0x7f) | 0x80) << (8 * k); u >>= 7; k++; }
    n = k + 1;
    return r | (u << (8 * k));
}
__device__ __forceinline__ uint32_t byte_of(uint64_t lo, uint64_t hi, int q) {
    return (uint32_t)((q < 8 ? lo >> (8 * q) : hi >> (8 * (q - 8))) & 0xffu);
}
__global__ void __launch_bounds__(M_NT)
k_mhint(const MEnt* __restrict__ e, const MCopy* __restrict__ cp, const cly_tuple* __restrict__ tup,
        const uint4* __restrict__ keys, const uint32_t* __restrict__ hsz, const MSum* __restrict__ bsum,
        const MTot* tot, uint64_t stride, uint8_t* hint, uint64_t hint_cap) {
    __shared__ uint32_t t4[1024];
    __shared__ MSum sh[M_NT / 64];
    __shared__ __attribute__((aligned(16))) uint8_t buf[MH_BUF + 48];
    crc_table4_init(t4);
    const uint64_t nl = tot->nl;
    const uint64_t b0 = (uint64_t)blockIdx.x * M_BLK;
    MSum carry = bsum[blockIdx.x];
    for (int it = 0; it < M_IT; it++) {
        if (b0 + (uint64_t)it * M_NT >= nl) break;              // (uniform)
        const uint64_t j = b0 + (uint64_t)it * M_NT + threadIdx.x;
        const uint32_t hs = j < nl ? hsz[j] : 0;
        MSum v = {hs, 0};
        MSum total;
        const MSum ex = block_excl(v, total, sh);
        const uint64_t H0 = carry.bytes;
        const uint64_t ho = H0 + ex.bytes;
        carry.bytes += total.bytes;
        const bool staged = total.bytes <= MH_BUF;              // (uniform)
        const uint32_t ph = (uint32_t)((uintptr_t)(hint + H0) & 15u);   // the stage's 16-B phase
        const uint32_t o = ph + (uint32_t)(ho - H0);            // the record's stage offset
        const bool mine = j < nl && ho + hs <= hint_cap;
        uint32_t s = 0xFFFFFFFFu;
        if (mine) {
            // the copy descriptor locates the realKey (its first MH_KEY bytes
            // are in keys[j], kept by k_mcopy); the tuple only for keys of 64 KiB on
            const MCopy c = cp[j];
            const uint8_t* rkey = (const uint8_t*)c.src + MC_KOFF(c.pre);
            uint32_t rk = MC_RK(c.pre);
            if (rk == 0xFFFFu) {
                const cly_tuple t = tup[e[j].tuple];
                rk = t.key_size - t.txid_len;
            }
            const uint4 k4 = rk <= MH_KEY ? keys[j] : make_uint4(0, 0, 0, 0);
            const uint64_t fid = c.dst / stride, off = c.dst - fid * stride;
            int nf, nofs, nk;
            const uint64_t pf = uv_pack(zz((int64_t)fid), nf), po = uv_pack(zz((int64_t)off), nofs);
            const int pl = nf + nofs;                            // <= 10
            const uint64_t pvl = nf < 8 ? pf | (po << (8 * nf)) : pf;
            const uint64_t pvh = nf < 8 ? (nf ? po >> (64 - 8 * nf) : 0) : po;   // (nf >= 1)
            const uint64_t kv = uv_pack(zz((int64_t)rk), nk);    // nk <= 5
            // header bytes 0..n-1 (crc bytes 0..3 later): 0 0 varint(rk) 2pl 0
            const int n = 8 + nk;
            uint64_t hl = kv << 48, hh = kv >> 16;
            const uint64_t tailb = (uint64_t)(2 * pl);           // varint(zz(pl)): one byte
            if (6 + nk < 8) hl |= tailb << (8 * (6 + nk)); else hh |= tailb << (8 * (6 + nk - 8));
            auto put = [&](uint32_t q, uint32_t bv) {
                if (staged) buf[o + q] = (uint8_t)bv;
                else { hint[ho + q] = (uint8_t)bv; s = crc_upd(t4, s, bv); }
            };
            #pragma unroll
            for (int q = 4; q < 14; q++)
                if (q < n) put((uint32_t)q, byte_of(hl, hh, q));
            if (rk <= MH_KEY) {
                // realKey from k_mcopy's copy
                const uint32_t kd[4] = {k4.x, k4.y, k4.z, k4.w};
                #pragma unroll
                for (int q = 0; q < MH_KEY; q++)
                    if ((uint32_t)q < rk) put((uint32_t)n + q, (kd[q >> 2] >> (8 * (q & 3))) & 0xffu);
            } else {
                // realKey: aligned dwords holding its bytes, shifted into place
                const uintptr_t ka = (uintptr_t)rkey;
                const CLY_GLB uint32_t* kw = (const CLY_GLB uint32_t*)(ka & ~(uintptr_t)3);
                const uint32_t kb = (uint32_t)(ka & 3);
                uint32_t prev = kw[0];
                for (uint32_t q = 0, k = 0; q < rk; q += 4, k++) {
                    const uint32_t nxt = 4 * (k + 1) < kb + rk ? kw[k + 1] : 0u;
                    const uint32_t x = __builtin_amdgcn_alignbit(nxt, prev, 8 * kb);
                    #pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (q + i < rk) put((uint32_t)n + q + i, (x >> (8 * i)) & 0xffu);
                    prev = nxt;
                }
            }
            #pragma unroll
            for (int q = 0; q < 10; q++)
                if (q < pl) put((uint32_t)n + rk + q, byte_of(pvl, pvh, q));
        }
        if (staged) {
            __syncthreads();
            if (mine) {
                // CRC of bytes 4 .. hs-1 from the stage: aligned dword reads, shifted
                const uint32_t bb = o + 4, sh8 = 8 * (bb & 3);
                const uint32_t* w = (const uint32_t*)(buf + (bb & ~3u));
                const uint32_t nb = hs - 4, nw = nb >> 2;
                uint32_t w0 = w[0];
                uint32_t k = 0;
                for (; k < nw; k++) {
                    const uint32_t w1 = w[k + 1];
                    const uint32_t x = s ^ __builtin_amdgcn_alignbit(w1, w0, sh8);
                    s = t4[768 + (x & 0xff)] ^ t4[512 + ((x >> 8) & 0xff)] ^ t4[256 + ((x >> 16) & 0xff)] ^ t4[x >> 24];
                    w0 = w1;
                }
                const uint32_t x = __builtin_amdgcn_alignbit(w[k + 1], w0, sh8);
                #pragma unroll
                for (int i = 0; i < 3; i++)
                    if ((uint32_t)i < (nb & 3u)) s = crc_upd(t4, s, (x >> (8 * i)) & 0xffu);
            }
        }
        if (mine) {
            s = ~s;
            #pragma unroll
            for (int q = 0; q < 4; q++) {
                if (staged) buf[o + q] = (uint8_t)(s >> (8 * q));
                else hint[ho + q] = (uint8_t)(s >> (8 * q));
            }
        }
        if (staged) {
            __syncthreads();
            uint64_t H1 = H0 + total.bytes;
            if (H1 > hint_cap) H1 = hint_cap;
            if (H1 > H0) {
                // 16-B chunks of [H0 - ph, H1): whole ones with one store, the two
                // partial ones byte by byte
                const uint64_t C0 = H0 - ph, nch = (H1 - C0 + 15) >> 4;
                for (uint64_t ci = threadIdx.x; ci < nch; ci += M_NT) {
                    const uint64_t c = C0 + 16 * ci;
                    const uint32_t lo = (uint32_t)(16 * ci);
                    if (c >= H0 && c + 16 <= H1) {
                        *(uint4*)(hint + c) = *(const uint4*)(buf + lo);
                    } else {
                        for (int q = 0; q < 16; q++)
                            if (c + q >= H0 && c + q < H1) hint[c + q] = buf[lo + q];
                    }
                }
            }
            __syncthreads();
        }
    }
}

// ---- k_mcopy: one 4-KiB destination block per wave ---------------------------
// The wave loads the copy descriptors of the records covering its block into
// LDS and builds the block's piece map: for each 16-B piece, the last record
// starting at or before it (each record marks the first piece at or after its
// start with an LDS max, then a prefix max over the 256 pieces: four per lane
// plus a DPP max-scan across the wave).  Lane l then writes pieces l, l+64,
// l+128, l+192 (each store instruction covers 1 KiB): a piece inside one
// record's body is one dwordx4 load at a dword-aligned address (+ one dword
// when the source is not dword-aligned) funnel-shifted into place, all issued
// before any store; a lane's first piece across two records is assembled
// from two partial loads; any other piece (more than one boundary, a
// re-encoded prefix, the end of the file, an append's kept bytes) gathers its
// 16 bytes one by one.
__device__ const uint8_t g_zero_byte = 0;
__device__ const uint32_t g_zero_words[4] = {0u, 0u, 0u, 0u};
typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));   // 16 B, dword-aligned
typedef uint32_t mc_u32x4 __attribute__((ext_vector_type(4)));
#define MC_W 4                                   // waves per workgroup
#define MC_P (M_CB / 16 / 64)                    // pieces per lane
#define MC_NPIECE (M_CB / 16)
__device__ __forceinline__ void mc_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// n bytes (0 < n <= 16) from byte address s as 16 bytes (bytes from n on
// undefined): only the dwords that hold one of the n bytes are loaded.
__device__ __forceinline__ void mc_part(uint64_t s, int n, uint32_t (&w)[4]) {
    const CLY_GLB uint32_t* wp = (const CLY_GLB uint32_t*)(s & ~3ull);
    const uint32_t sh = (uint32_t)(s & 3);
    const int nd = (int)((sh + (uint32_t)n + 3) >> 2);
    uint32_t t[5];
    #pragma unroll
    for (int q = 0; q < 5; q++) t[q] = q < nd ? wp[q] : 0u;
    #pragma unroll
    for (int q = 0; q < 4; q++) w[q] = __builtin_amdgcn_alignbit(t[q + 1], t[q], sh * 8);
}
// the same in two halves: the loads (issued with no branch: a lane that needs
// none, or fewer than five dwords, loads zero words), then the funnel shift
__device__ __forceinline__ void mc_load(uint64_t s, int n, bool on, uint32_t (&t)[5]) {
    const CLY_GLB uint32_t* wp = (const CLY_GLB uint32_t*)(s & ~3ull);
    const int nd = on ? (int)(((uint32_t)(s & 3) + (uint32_t)n + 3) >> 2) : 0;
    #pragma unroll
    for (int q = 0; q < 5; q++) t[q] = *(q < nd ? wp + q : (const CLY_GLB uint32_t*)g_zero_words);
}
__device__ __forceinline__ void mc_align(const uint32_t (&t)[5], uint64_t s, uint32_t (&w)[4]) {
    const uint32_t sh = (uint32_t)(s & 3) * 8;
    #pragma unroll
    for (int q = 0; q < 4; q++) w[q] = __builtin_amdgcn_alignbit(t[q + 1], t[q], sh);
}
__device__ __forceinline__ uint32_t mc_sel(const uint32_t (&b)[4], int k) {
    return k == 0 ? b[0] : k == 1 ? b[1] : k == 2 ? b[2] : k == 3 ? b[3] : 0u;
}
// 16 bytes: x[0..nA) then y[0..16-nA)
__device__ __forceinline__ void mc_join(const uint32_t (&x)[4], const uint32_t (&y)[4], int nA, uint32_t (&o)[4]) {
    const int m = nA >> 2, r = nA & 3;
    #pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t hi = mc_sel(y, j - m), lo = mc_sel(y, j - m - 1);
        const uint32_t sj = r ? __builtin_amdgcn_alignbit(hi, lo, 32 - 8 * r) : hi;     // (y << 8 nA), dword j
        const int kb = nA - 4 * j;                                                       // bytes of x in dword j
        const uint32_t mk = kb >= 4 ? 0xFFFFFFFFu : kb <= 0 ? 0u : (1u << (8 * kb)) - 1u;
        o[j] = (x[j] & mk) | (sj & ~mk);
    }
}
template <int CTRL, int RM = 0xf>
__device__ __forceinline__ uint32_t mc_dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, RM, 0xf, false);
}
// inclusive max over the wave (DPP row shifts and row broadcasts; 0 = identity)
__device__ __forceinline__ uint32_t mc_wave_max_incl(uint32_t v) {
    v = max(v, mc_dpp<0x111>(v));
    v = max(v, mc_dpp<0x112>(v));
    v = max(v, mc_dpp<0x114>(v));
    v = max(v, mc_dpp<0x118>(v));
    v = max(v, mc_dpp<0x142, 0xa>(v));
    v = max(v, mc_dpp<0x143, 0xc>(v));
    return v;
}

// A destination block's place: its region's end L and kept prefix, its first
// descriptor j0 and descriptor count (ok = false: nothing of it is written).
struct McBlk { bool ok; uint32_t j0, cnt; uint64_t fo, L, keep; };
// lanes 0 and 1: bmap[b + lane], and flen[k] (lane 0) / fstart[k + 1] (lane 1)
__device__ __forceinline__ void mc_info_load(uint64_t b, uint64_t nblocks, uint64_t bpf, const uint32_t* bmap,
                                             const uint64_t* fstart, const uint64_t* flen, int lane, uint32_t& vb,
                                             uint64_t& vf) {
    vb = 0u; vf = 0u;
    if (b < nblocks && lane < 2) {
        const uint64_t k = b / bpf;
        vb = bmap[b + (uint64_t)lane];
        vf = lane ? fstart[k + 1] : flen[k];
    }
}
// the loaded descriptor's registers are needed here (the compiler's wait for them)
__device__ __forceinline__ void mc_pin(const MCopy& c) {
    asm volatile("" ::"v"(c.dst), "v"(c.src), "v"(c.size), "v"(c.pre));
}
template <int CMAX>
__device__ __forceinline__ McBlk mc_info_use(uint64_t b, uint64_t nblocks, uint64_t bpf, uint64_t stride, uint64_t lo0,
                                             uint32_t vb, uint64_t vf) {
    McBlk r;
    r.ok = false; r.j0 = 0; r.cnt = 0; r.fo = 0; r.L = 0; r.keep = 0;
    if (b >= nblocks) return r;
    const uint64_t k = b / bpf;
    r.fo = b * M_CB - k * stride;
    r.L = ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(vf >> 32), 0) << 32) | __builtin_amdgcn_readlane((uint32_t)vf, 0);
    r.keep = k == 0 ? lo0 : 0;
    if (r.fo >= r.L || r.fo + M_CB <= r.keep || r.L <= r.keep) return r;
    r.j0 = __builtin_amdgcn_readlane(vb, 0);
    uint64_t j1 = ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(vf >> 32), 1) << 32) | __builtin_amdgcn_readlane((uint32_t)vf, 1);
    if (r.fo + M_CB < r.L) j1 = (uint64_t)__builtin_amdgcn_readlane(vb, 1) + 1;
    const uint64_t n = j1 - r.j0;
    r.cnt = n > (uint64_t)CMAX ? (uint32_t)CMAX : (uint32_t)n;
    r.ok = true;
    return r;
}

// Template over the descriptor capacity per block (CMAX) and the prefix stride
// (PRE); lo0 = first byte of region 0 that belongs to the output (appends
// continue an active file: bytes below it are kept as they are).  fstart[k]
// is the first descriptor of region k; flen[k] the region's end offset.
template <int CMAX, int PRE, bool TWO>
__global__ void __launch_bounds__(64 * MC_W, 4)
k_mcopy(const MCopy* __restrict__ cp, const uint8_t* __restrict__ pre, const uint32_t* __restrict__ bmap,
        const uint64_t* __restrict__ fstart, const uint64_t* __restrict__ flen, uint64_t stride,
        uint64_t nblocks, uint8_t* out, uint64_t lo0, uint4* keys) {
    __shared__ mc_u32x4 s_desc[MC_W][CMAX];              // source (lo, hi), rel (dst - block start), size
    __shared__ uint8_t s_pre[MC_W][CMAX];
    __shared__ mc_u32x4 s_map[MC_W][MC_NPIECE / 4];      // piece -> descriptor
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;   // (scalar: block indices in SGPRs)
    mc_u32x4* desc = s_desc[w];
    uint8_t* pres = s_pre[w];
    uint32_t* map = (uint32_t*)s_map[w];
    const uint64_t bpf = stride / M_CB, step = (uint64_t)gridDim.x * MC_W;
    // A block's loads depend on each other (bmap -> descriptors -> source
    // bytes).  The wave loads its next block's descriptors (the first 64, one
    // per lane) and the bmap / flen / fstart words of the block after that
    // while it copies the current block, as vector loads issued before the
    // block's source loads: one wait for those (vmcnt counts loads and stores
    // in issue order) finds all of them in, before any store of the block.
    uint64_t b = (uint64_t)blockIdx.x * MC_W + w;
    uint32_t vb;
    uint64_t vf;
    mc_info_load(b, nblocks, bpf, bmap, fstart, flen, lane, vb, vf);
    McBlk cur = mc_info_use<CMAX>(b, nblocks, bpf, stride, lo0, vb, vf);
    MCopy cq = {0, 0, 0, 0};
    if (cur.ok && (uint32_t)lane < cur.cnt) cq = cp[cur.j0 + lane];
    mc_info_load(b + step, nblocks, bpf, bmap, fstart, flen, lane, vb, vf);
    McBlk nx = mc_info_use<CMAX>(b + step, nblocks, bpf, stride, lo0, vb, vf);
    mc_pin(cq);
    for (; b < nblocks; b += step) {
        MCopy cn = {0, 0, 0, 0};
        if (nx.ok && (uint32_t)lane < nx.cnt) cn = cp[nx.j0 + lane];
        mc_info_load(b + 2 * step, nblocks, bpf, bmap, fstart, flen, lane, vb, vf);
        const MCopy cl = cq;
        const McBlk cb = cur;
        McBlk nx2;
        if (!cb.ok) {                                           // (wave-uniform)
            mc_pin(cn);
            nx2 = mc_info_use<CMAX>(b + 2 * step, nblocks, bpf, stride, lo0, vb, vf);
            cur = nx; cq = cn; nx = nx2;
            continue;
        }
        const uint64_t B = b * M_CB, fo = cb.fo, L = cb.L, keep = cb.keep;
        const uint32_t j0 = cb.j0, cnt = cb.cnt;
        mc_wave_sync();                                         // previous block's readers are done
        s_map[w][lane] = (mc_u32x4){0u, 0u, 0u, 0u};
        mc_wave_sync();
        for (uint32_t q = lane; q < cnt; q += 64) {
            const MCopy c = q < 64 ? cl : cp[j0 + q];
            const int32_t rel = (int32_t)((int64_t)c.dst - (int64_t)B);   // >= -(record size) > -2^31
            desc[q] = (mc_u32x4){(uint32_t)c.src, (uint32_t)(c.src >> 32), (uint32_t)rel, c.size};
            pres[q] = (uint8_t)c.pre;
            const int32_t pi = rel <= 0 ? 0 : (rel + 15) >> 4;  // the first piece at or after the record's start
            if (pi < MC_NPIECE) __atomic_fetch_max(map + pi, q, __ATOMIC_RELAXED);
        }
        mc_wave_sync();
        {
            mc_u32x4 v = s_map[w][lane];
            v.y = max(v.y, v.x); v.z = max(v.z, v.y); v.w = max(v.w, v.z);
            const uint32_t incl = mc_wave_max_incl(v.w);
            const uint32_t ex = mc_dpp<0x138>(incl);            // lane - 1's (lane 0: 0)
            v.x = max(v.x, ex); v.y = max(v.y, ex); v.z = max(v.z, ex); v.w = max(v.w, ex);
            s_map[w][lane] = v;
        }
        mc_wave_sync();
        const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(out + B, (short)0, (int)M_CB, 0x00020000);
        uint32_t a[MC_P][5];
        uint32_t fast = 0, slow = 0, shs = 0;
        // (branch-free: every lane loads every piece, a piece that is not a
        // fast one from a zero word, so that the loads land in a[][] directly
        // and all of them are in flight together)
        #pragma unroll
        for (int p = 0; p < MC_P; p++) {
            const int P = p * 64 + lane, d = P * 16;
            const bool out_ = fo + (uint64_t)d >= L || fo + (uint64_t)d + 16 <= keep;
            const bool kept = fo + (uint64_t)d < keep;
            const uint32_t r = map[P];
            const mc_u32x4 D = desc[r];
            const int r0 = d - (int32_t)D.z, pr = pres[r];
            const bool isf = !out_ && !kept && r0 >= pr && (int64_t)r0 + 16 <= (int64_t)D.w;
            const uint64_t sa = isf ? (((uint64_t)D.y << 32) | D.x) + (uint64_t)(r0 - pr) : (uint64_t)g_zero_words;
            const CLY_GLB uint32_t* wp = (const CLY_GLB uint32_t*)(sa & ~3ull);
            const u32x4a v4 = *(const CLY_GLB u32x4a*)wp;      // one dwordx4 at a dword-aligned address
            a[p][0] = v4.x; a[p][1] = v4.y; a[p][2] = v4.z; a[p][3] = v4.w;
            a[p][4] = wp[(sa & 3) ? 4 : 0];                      // (dword 0 again when not needed)
            fast |= (isf ? 1u : 0u) << p;
            slow |= (!out_ && !isf ? 1u : 0u) << p;
            shs |= (uint32_t)(sa & 3) << (2 * p);
        }
        // the lane's first slow piece: across exactly one record boundary, the
        // tail of record r (body or prefix) then the head of record r + 1
        uint32_t ta[5], tb[5];
        uint64_t sA = 0, sB = 0;
        int d2 = -1, n2 = 0;                                    // the piece assembled from two records
        if (TWO) {
          bool two = false;
          int nA = 0, d = 0;
          if (slow) {
            const int p = __builtin_ctz(slow);
            const int P = p * 64 + lane;
            d = P * 16;
            two = fo + (uint64_t)d >= keep && fo + (uint64_t)d + 16 <= L;
            const uint32_t r = two ? map[P] : 0u;
            two = two && r + 1 < cnt;
            if (two) {
                const mc_u32x4 D = desc[r], E = desc[r + 1];
                const int r0 = d - (int32_t)D.z, pr = pres[r], pb = pres[r + 1];
                nA = (int)D.w - r0;
                two = nA > 0 && nA < 16 && (int32_t)E.z == d + nA && (int)E.w >= 16 - nA;
                if (r0 >= pr) sA = (((uint64_t)D.y << 32) | D.x) + (uint64_t)(r0 - pr);
                else if (r0 + nA <= pr) sA = (uint64_t)(pre + (uint64_t)(j0 + r) * PRE + r0);
                else two = false;
                if (pb == 0) sB = ((uint64_t)E.y << 32) | E.x;
                else if (pb >= 16 - nA) sB = (uint64_t)(pre + (uint64_t)(j0 + r + 1) * PRE);
                else two = false;
            }
          }
          mc_load(sA, nA, two, ta);
          mc_load(sB, 16 - nA, two, tb);
          if (two) { d2 = d; n2 = nA; }
        }
        // the merge's hint records: the first MH_KEY realKey bytes of every
        // record starting in the block, re-read from the source lines the
        // block's loads bring into L2 (k_mhint then reads 16 B per record
        // instead of a line of the file); the first 64 records' loads here
        uint32_t tk[5];
        uint64_t sk = 0;
        bool kst = false;
        if (keys) {
            bool kon = false;
            if ((uint32_t)lane < cnt) {
                const mc_u32x4 D = desc[lane];
                if ((int32_t)D.z >= 0 && (int32_t)D.z < M_CB && MC_RK(cl.pre) <= MH_KEY) {   // starts in the block
                    kst = true;
                    kon = MC_RK(cl.pre) != 0;
                    sk = (((uint64_t)D.y << 32) | D.x) + MC_KOFF(cl.pre);
                }
            }
            mc_load(sk, (int)MC_RK(cl.pre), kon, tk);
        }
        // the block's loads are in, and with them the next blocks' descriptors
        // and words (issued before them)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        mc_pin(cn);
        nx2 = mc_info_use<CMAX>(b + 2 * step, nblocks, bpf, stride, lo0, vb, vf);
        cur = nx; cq = cn; nx = nx2;
        if (TWO && d2 >= 0) {
            uint32_t xa[4], xb[4], o[4];
            mc_align(ta, sA, xa);
            mc_align(tb, sB, xb);
            mc_join(xa, xb, n2, o);
            __builtin_amdgcn_raw_buffer_store_b128((mc_u32x4){o[0], o[1], o[2], o[3]}, ors, d2, 0, 0);
            slow &= slow - 1;
        }
        #pragma unroll
        for (int p = 0; p < MC_P; p++) {
            if (!(fast & (1u << p))) continue;
            const int d = (p * 64 + lane) * 16;
            const uint32_t sh = ((shs >> (2 * p)) & 3) * 8;
            mc_u32x4 o;
            o.x = __builtin_amdgcn_alignbit(a[p][1], a[p][0], sh);
            o.y = __builtin_amdgcn_alignbit(a[p][2], a[p][1], sh);
            o.z = __builtin_amdgcn_alignbit(a[p][3], a[p][2], sh);
            o.w = __builtin_amdgcn_alignbit(a[p][4], a[p][3], sh);
            __builtin_amdgcn_raw_buffer_store_b128(o, ors, d, 0, 0);
        }
        // gather pieces: byte q from its record (re-encoded prefix, body) or zero
        // past the file end; the 16 loads of a piece are issued together
        #pragma unroll 1
        while (slow) {
            const int p = __builtin_ctz(slow);
            slow &= slow - 1;
            const int d = (p * 64 + lane) * 16;
            int jj = (int)map[d >> 4];
            const uint8_t* bp[16];
            #pragma unroll
            for (int q = 0; q < 16; q++) {
                const int pos = d + q;
                while (jj + 1 < (int)cnt && (int32_t)desc[jj + 1].z <= pos) jj++;
                const mc_u32x4 D = desc[jj];
                const int r = pos - (int32_t)D.z;
                const uint8_t* ptr = &g_zero_byte;
                if (fo + (uint64_t)pos < keep) {
                    ptr = out + B + pos;                        // an active file's existing bytes
                } else if (fo + (uint64_t)pos < L && r >= 0 && (uint32_t)r < D.w) {
                    const int pj = pres[jj];
                    ptr = r < pj ? pre + (uint64_t)(j0 + jj) * PRE + r
                                 : (const uint8_t*)(((uint64_t)D.y << 32) | D.x) + (r - pj);
                }
                bp[q] = ptr;
            }
            uint32_t v[4] = {0, 0, 0, 0};
            #pragma unroll
            for (int q = 0; q < 16; q++) v[q >> 2] |= (uint32_t)*bp[q] << (8 * (q & 3));
            *(uint4*)(out + B + d) = make_uint4(v[0], v[1], v[2], v[3]);
        }
        if (keys) {
            if (kst) {
                uint32_t kw[4];
                mc_align(tk, sk, kw);
                keys[j0 + lane] = make_uint4(kw[0], kw[1], kw[2], kw[3]);
            }
            for (uint32_t q = lane + 64; q < cnt; q += 64) {
                const int32_t rl = (int32_t)desc[q].z;
                if (rl < 0 || rl >= M_CB) continue;                  // starts in another block
                const uint32_t px = cp[j0 + q].pre;
                if (MC_RK(px) > MH_KEY) continue;
                const mc_u32x4 D = desc[q];
                uint32_t kw[4];
                kw[0] = kw[1] = kw[2] = kw[3] = 0u;
                if (MC_RK(px)) mc_part((((uint64_t)D.y << 32) | D.x) + MC_KOFF(px), (int)MC_RK(px), kw);   // (its bytes only)
                keys[j0 + q] = make_uint4(kw[0], kw[1], kw[2], kw[3]);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// CLY_MERGE_DEBUG=1: synchronise after every kernel and name the one that failed
static int merge_debug() {
    static int v = -1;
    if (v < 0) { const char* e = getenv("CLY_MERGE_DEBUG"); v = e && *e == '1'; }
    return v;
}
#define MDBG(st, name) do { if (merge_debug()) { hipError_t e_ = hipStreamSynchronize(st); \
    if (e_ == hipSuccess) e_ = hipGetLastError(); \
    fprintf(stderr, "clymerge: %s -> %s\n", name, hipGetErrorString(e_)); \
    if (e_ != hipSuccess) { rc = CLY_ERR_DEVICE; goto done; } } } while (0)

extern "C" int cly_merge_device(cly_ctx* ctx, const cly_file* files, int nfiles, const cly_tuple* d_tuples,
                                const uint64_t* file_first, const cly_file_result* res, const uint8_t* d_live,
                                uint64_t data_file_size, uint8_t* d_out, uint32_t out_max_files,
                                uint64_t* out_file_len, uint8_t* d_hint, uint64_t hint_cap,
                                cly_merge_result* mres, void* stream_v) {
    if (!ctx || !mres || nfiles < 0 || (nfiles && (!files || !file_first || !res)) || data_file_size == 0)
        return CLY_ERR_ARG;
    memset(mres, 0, sizeof(*mres));
    const uint64_t stride = (data_file_size + M_CB - 1) / M_CB * M_CB;
    mres->out_stride = stride;
    // the reference's merge stops with the scan's error (merge.go:94-99)
    uint64_t T = 0;
    for (int i = 0; i < nfiles; i++) {
        if (res[i].status < 0) return res[i].status;
        if (file_first[i] != T) return CLY_ERR_ARG;             // tuples of the files back to back
        T += res[i].n_records;
    }
    if (T >= (1ull << 32)) return CLY_ERR_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return CLY_ERR_DEVICE;
    hipStream_t st = stream_v ? (hipStream_t)stream_v : ctx->stream;
    int rc = CLY_OK;
    uint64_t* h_fb = (uint64_t*)malloc(sizeof(uint64_t) * (2 * (size_t)nfiles + 2));
    uint64_t *d_fb = nullptr, *d_plan = nullptr, *d_fstart = nullptr, *d_flen = nullptr, *d_pk = nullptr, *d_pkc = nullptr;
    MSum* d_bsum = nullptr;
    MEnt* d_ent = nullptr;
    MCopy* d_cp = nullptr;
    uint8_t* d_pre = nullptr;
    uint32_t *d_bmap = nullptr, *d_hsz = nullptr;
    uint4* d_keys = nullptr;
    MTot* d_tot = nullptr;
    MTot h_tot;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const uint64_t nblk = T / M_BLK + 1;
    CLY_CKG(hipEventCreateWithFlags(&e0, hipEventDisableSystemFence));     // (timing only)
    CLY_CKG(hipEventCreateWithFlags(&e1, hipEventDisableSystemFence));
    for (int i = 0; i < nfiles; i++) h_fb[i] = file_first[i];
    h_fb[nfiles] = T;
    for (int i = 0; i < nfiles; i++) h_fb[nfiles + 1 + i] = (uint64_t)files[i].base;
    CLY_CKG(cly_scratch(ctx, MS_FB, sizeof(uint64_t) * (2 * (size_t)nfiles + 2), &d_fb));
    CLY_CKG(hipMemcpyAsync(d_fb, h_fb, sizeof(uint64_t) * (2 * (size_t)nfiles + 1), hipMemcpyHostToDevice, st));
    CLY_CKG(cly_scratch(ctx, MS_TOT, sizeof(MTot), &d_tot));
    CLY_CKG(hipMemsetAsync(d_tot, 0, sizeof(MTot), st));
    CLY_CKG(cly_scratch(ctx, MS_PLAN, sizeof(uint64_t) * (T + 1), &d_plan));
    CLY_CKG(cly_scratch(ctx, MS_BSUM, sizeof(MSum) * nblk, &d_bsum));
    CLY_CKG(cly_scratch(ctx, MS_ENT, sizeof(MEnt) * (T + 1), &d_ent));
    CLY_CKG(cly_scratch(ctx, MS_PK, sizeof(uint64_t) * (T + 1), &d_pk));
    CLY_CKG(cly_scratch(ctx, MS_PKC, sizeof(uint64_t) * (T + 1), &d_pkc));
    CLY_CKG(hipEventRecord(e0, st));
    if (T) {
        k_mplan<<<(unsigned)nblk, M_NT, 0, st>>>(d_tuples, T, d_live, d_fb, d_fb + nfiles + 1, nfiles, d_plan, d_pk, d_bsum,
                                                  data_file_size, d_tot);
        MDBG(st, "k_mplan");
        k_msums<<<1, M_NT, 0, st>>>(d_bsum, nblk, &d_tot->bytes, &d_tot->nl);
        MDBG(st, "k_msums");
        k_mcompact<<<(unsigned)nblk, M_NT, 0, st>>>(d_plan, d_pk, T, d_bsum, d_ent, d_pkc);
        MDBG(st, "k_mcompact");
    }
    CLY_CKG(hipMemcpyAsync(&h_tot, d_tot, sizeof(MTot), hipMemcpyDeviceToHost, st));
    CLY_CKG(hipStreamSynchronize(st));
    if (h_tot.bad & 1) { rc = CLY_ERR_VARINT; goto done; }
    if (h_tot.bad & 2) { rc = CLY_ERR_ARG; goto done; }
    mres->n_live = h_tot.nl;
    if (h_tot.nl == 0) goto timing;
    {
        // n_out <= 2 total / dfs + 2: two neighbouring files hold more than dfs bytes
        uint64_t fcap64 = 2 * h_tot.bytes / data_file_size + 4;
        if (fcap64 > h_tot.nl + 2) fcap64 = h_tot.nl + 2;
        const uint32_t fcap = (uint32_t)fcap64;
        CLY_CKG(cly_scratch(ctx, MS_FSTART, sizeof(uint64_t) * (fcap + 1), &d_fstart));
        CLY_CKG(cly_scratch(ctx, MS_FLEN, sizeof(uint64_t) * (fcap + 1), &d_flen));
        k_mrot<<<1, M_ROT, 0, st>>>(d_ent, d_tot, data_file_size, fcap, d_fstart, d_flen);
        MDBG(st, "k_mrot");
        CLY_CKG(hipMemcpyAsync(&h_tot, d_tot, sizeof(MTot), hipMemcpyDeviceToHost, st));
        CLY_CKG(hipStreamSynchronize(st));
        mres->n_out_files = h_tot.n_out;
        if (h_tot.n_out >= fcap) { rc = CLY_ERR_DEVICE; goto done; }   // cannot happen (bound above)
        const uint64_t nl = h_tot.nl;
        const uint64_t lblk = nl / M_BLK + 1;
        const uint64_t nblocks = (uint64_t)h_tot.n_out * (stride / M_CB);
        if (lblk > nblk) { rc = CLY_ERR_DEVICE; goto done; }    // cannot happen: nl <= T
        CLY_CKG(cly_scratch(ctx, MS_CP, sizeof(MCopy) * nl, &d_cp));
        CLY_CKG(cly_scratch(ctx, MS_PRE, (size_t)M_PRE * nl, &d_pre));
        CLY_CKG(cly_scratch(ctx, MS_BMAP, sizeof(uint32_t) * (nblocks + 1), &d_bmap));
        CLY_CKG(cly_scratch(ctx, MS_HSZ, sizeof(uint32_t) * nl, &d_hsz));
        k_mplace<<<(unsigned)lblk, M_NT, 0, st>>>(d_ent, d_pkc, d_tuples, d_plan, d_fb, d_fb + nfiles + 1, nfiles, d_fstart,
                                                   d_tot, stride, d_cp, d_pre, d_bmap, d_hsz, d_bsum);
        MDBG(st, "k_mplace");
        k_msums<<<1, M_NT, 0, st>>>(d_bsum, lblk, &d_tot->hint_bytes, nullptr);
        CLY_CKG(hipMemcpyAsync(&h_tot, d_tot, sizeof(MTot), hipMemcpyDeviceToHost, st));
        CLY_CKG(hipStreamSynchronize(st));
        mres->hint_bytes = h_tot.hint_bytes;
        mres->n_reencoded = h_tot.n_re;
        if (h_tot.n_out > out_max_files || !d_out || h_tot.hint_bytes > hint_cap || !d_hint) {
            rc = CLY_ERR_CAPACITY;
            goto done;
        }
        CLY_CKG(cly_scratch(ctx, MS_KEYS, sizeof(uint4) * nl, &d_keys));
        const uint64_t wgs = (nblocks + MC_W - 1) / MC_W;
        unsigned grid = wgs < 16384 ? (unsigned)wgs : 16384u;
        k_mcopy<M_CMAX, M_PRE, true><<<grid, 64 * MC_W, 0, st>>>(d_cp, d_pre, d_bmap, d_fstart, d_flen, stride, nblocks,
                                                          d_out, 0, d_keys);
        MDBG(st, "k_mcopy");
        k_mhint<<<(unsigned)lblk, M_NT, 0, st>>>(d_ent, d_cp, d_tuples, d_keys, d_hsz, d_bsum, d_tot, stride, d_hint,
                                                  hint_cap);
        MDBG(st, "k_mhint");
        CLY_CKG(hipGetLastError());
        if (out_file_len) CLY_CKG(hipMemcpyAsync(out_file_len, d_flen, sizeof(uint64_t) * h_tot.n_out,
                                                 hipMemcpyDeviceToHost, st));
    }
timing:
    CLY_CKG(hipEventRecord(e1, st));
    CLY_CKG(hipEventSynchronize(e1));
    {
        float ms = 0;
        CLY_CKG(hipEventElapsedTime(&ms, e0, e1));
        mres->merge_ms = ms;
    }
done:
    hipStreamSynchronize(st);
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    free(h_fb);
    return rc;
}

// Host-memory entry (the cgo path): files in host memory (mmap), one live byte
// per record of the scan (scan order), merge data files and hint file back to
// host memory.  Scans the files on the device first (cly_scan_device).
extern "C" int cly_merge(cly_ctx* ctx, const cly_file* files, int nfiles, const uint8_t* live, uint64_t n_live_bytes,
                         uint64_t data_file_size, uint8_t* out, uint32_t out_max_files, uint64_t* out_file_len,
                         uint8_t* hint, uint64_t hint_cap, cly_merge_result* mres) {
    if (!ctx || !mres || nfiles < 0 || (nfiles && !files) || data_file_size == 0) return CLY_ERR_ARG;
    memset(mres, 0, sizeof(*mres));
    if (hipSetDevice(ctx->device) != hipSuccess) return CLY_ERR_DEVICE;
    hipStream_t st = ctx->stream;
    int rc = CLY_OK;
    const uint64_t stride = (data_file_size + M_CB - 1) / M_CB * M_CB;
    uint64_t total = 0;
    for (int i = 0; i < nfiles; i++) {
        if (files[i].len >= (1ULL << 32)) return CLY_ERR_ARG;
        total += (files[i].len + 4095) & ~4095ULL;
    }
    const int nf = nfiles ? nfiles : 1;
    cly_file* df = (cly_file*)calloc(nf, sizeof(cly_file));
    uint64_t* first = (uint64_t*)calloc(nf, sizeof(uint64_t));
    cly_file_result* res = (cly_file_result*)calloc(nf, sizeof(cly_file_result));
    uint8_t *d_bytes = nullptr, *d_live = nullptr, *d_out = nullptr, *d_hint = nullptr;
    cly_tuple* d_tup = nullptr;
    uint64_t need = 0, cap = 0, T = 0;
    CLY_CKG(hipMalloc((void**)&d_bytes, total + 4096));
    {
        uint64_t off = 0;
        for (int i = 0; i < nfiles; i++) {
            df[i] = files[i];
            df[i].base = d_bytes + off;
            if (files[i].len) CLY_CKG(hipMemcpyAsync(d_bytes + off, files[i].base, files[i].len, hipMemcpyHostToDevice, st));
            off += (files[i].len + 4095) & ~4095ULL;
        }
    }
    cap = cly_scan_capacity(files, nfiles) + 16;
    CLY_CKG(hipMalloc((void**)&d_tup, sizeof(cly_tuple) * cap));
    rc = cly_scan_device(ctx, df, nfiles, d_tup, cap, first, res, &need, nullptr, nullptr);
    if (rc == CLY_ERR_CAPACITY) {
        hipFree(d_tup);
        d_tup = nullptr;
        cap = need + 16;
        CLY_CKG(hipMalloc((void**)&d_tup, sizeof(cly_tuple) * cap));
        rc = cly_scan_device(ctx, df, nfiles, d_tup, cap, first, res, &need, nullptr, nullptr);
    }
    if (rc != CLY_OK) goto done;
    for (int i = 0; i < nfiles; i++) {
        if (res[i].status < 0) { rc = res[i].status; goto done; }
        T += res[i].n_records;
    }
    // tuples after a file's end may sit in the slots; the merge wants them back to back
    {
        uint64_t o = 0;
        for (int i = 0; i < nfiles; i++) {
            if (first[i] != o && res[i].n_records)
                CLY_CKG(hipMemcpyAsync(d_tup + o, d_tup + first[i], sizeof(cly_tuple) * res[i].n_records,
                                       hipMemcpyDeviceToDevice, st));
            first[i] = o;
            o += res[i].n_records;
        }
    }
    if (n_live_bytes != T || (T && !live)) { rc = CLY_ERR_ARG; goto done; }
    CLY_CKG(hipMalloc((void**)&d_live, T + 1));
    if (T) CLY_CKG(hipMemcpyAsync(d_live, live, T, hipMemcpyHostToDevice, st));
    if (out_max_files) CLY_CKG(hipMalloc((void**)&d_out, stride * out_max_files));
    if (hint_cap) CLY_CKG(hipMalloc((void**)&d_hint, hint_cap));
    rc = cly_merge_device(ctx, df, nfiles, d_tup, first, res, d_live, data_file_size, d_out, out_max_files,
                          out_file_len, d_hint, hint_cap, mres, nullptr);
    if (rc != CLY_OK) goto done;
    for (uint32_t k = 0; k < mres->n_out_files; k++)
        CLY_CKG(hipMemcpyAsync(out + k * stride, d_out + k * stride, out_file_len[k], hipMemcpyDeviceToHost, st));
    if (mres->hint_bytes) CLY_CKG(hipMemcpyAsync(hint, d_hint, mres->hint_bytes, hipMemcpyDeviceToHost, st));
    CLY_CKG(hipStreamSynchronize(st));
done:
    hipStreamSynchronize(st);
    hipFree(d_bytes); hipFree(d_tup); hipFree(d_live); hipFree(d_out); hipFree(d_hint);
    free(df); free(first); free(res);
    return rc;
}

// ---- hint-index load (loadIndexFromHintFile, merge.go:257-287) ---------------
// DecodeLogRecordPos (data/logRecord.go:126-134) over the records of a scanned
// hint file: Fid = uint32(Varint(value)), Offset = Varint(value[n:]).  A first
// varint that overflows makes the reference panic (buf[index:] with index < 0):
// the smallest such record index is reported.
__global__ void __launch_bounds__(256)
k_hintpos(const uint8_t* __restrict__ base, const cly_tuple* __restrict__ tup, uint64_t n, cly_pos* pos,
          unsigned long long* first_bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const cly_tuple t = tup[i];
        const uint8_t* v = base + t.offset + t.header_size + t.key_size;
        int n1 = 0, n2 = 0;
        const int64_t f = go_varint(v, (int64_t)t.value_size, n1);
        cly_pos p;
        p._pad = 0;
        if (n1 < 0) {
            atomicMin(first_bad, (unsigned long long)i);
            p.fid = 0;
            p.offset = 0;
        } else {
            p.fid = (uint32_t)f;
            p.offset = go_varint(v + n1, (int64_t)t.value_size - n1, n2);
        }
        pos[i] = p;
    }
}

extern "C" int cly_hint_positions_device(cly_ctx* ctx, const uint8_t* d_hint_file, const cly_tuple* d_tuples,
                                         uint64_t n, cly_pos* d_pos, uint64_t* first_bad, void* stream_v) {
    if (!ctx || (n && (!d_hint_file || !d_tuples || !d_pos))) return CLY_ERR_ARG;
    if (first_bad) *first_bad = n;
    if (!n) return CLY_OK;
    if (hipSetDevice(ctx->device) != hipSuccess) return CLY_ERR_DEVICE;
    hipStream_t st = stream_v ? (hipStream_t)stream_v : ctx->stream;
    int rc = CLY_OK;
    unsigned long long* d_bad = nullptr;
    unsigned long long h_bad = ~0ull;
    const uint64_t blocks = (n + 255) / 256;
    CLY_CKG(cly_scratch(ctx, MS_TOT, sizeof(MTot), &d_bad));
    CLY_CKG(hipMemcpyAsync(d_bad, &h_bad, sizeof(h_bad), hipMemcpyHostToDevice, st));
    k_hintpos<<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, st>>>(d_hint_file, d_tuples, n, d_pos, d_bad);
    CLY_CKG(hipGetLastError());
    CLY_CKG(hipMemcpyAsync(&h_bad, d_bad, sizeof(h_bad), hipMemcpyDeviceToHost, st));
    CLY_CKG(hipStreamSynchronize(st));
    if (h_bad < n) {
        if (first_bad) *first_bad = h_bad;
        rc = CLY_ERR_VARINT;
    }
done:
    return rc;
}

extern "C" int cly_hint_scan(cly_ctx* ctx, const cly_file* hint_file, cly_tuple* out, cly_pos* pos, uint64_t cap,
                             uint64_t* n_out, cly_file_result* res) {
    if (!ctx || !hint_file || !res || !n_out) return CLY_ERR_ARG;
    *n_out = 0;
    if (hipSetDevice(ctx->device) != hipSuccess) return CLY_ERR_DEVICE;
    hipStream_t st = ctx->stream;
    int rc = CLY_OK;
    uint8_t* d_bytes = nullptr;
    cly_tuple* d_tup = nullptr;
    cly_pos* d_pos = nullptr;
    cly_file df = *hint_file;
    uint64_t first = 0, need = 0, nrec = 0, bad = 0;
    const uint64_t tcap = cly_scan_capacity(hint_file, 1) + 16;
    CLY_CKG(hipMalloc((void**)&d_bytes, hint_file->len + 16));
    if (hint_file->len) CLY_CKG(hipMemcpyAsync(d_bytes, hint_file->base, hint_file->len, hipMemcpyHostToDevice, st));
    df.base = d_bytes;
    CLY_CKG(hipMalloc((void**)&d_tup, sizeof(cly_tuple) * tcap));
    rc = cly_scan_device(ctx, &df, 1, d_tup, tcap, &first, res, &need, nullptr, nullptr);
    if (rc != CLY_OK) goto done;
    nrec = res->n_records;
    if (nrec) {
        CLY_CKG(hipMalloc((void**)&d_pos, sizeof(cly_pos) * nrec));
        rc = cly_hint_positions_device(ctx, d_bytes, d_tup + first, nrec, d_pos, &bad, nullptr);
        if (rc == CLY_ERR_VARINT) nrec = bad;                  // the records before the panic
        else if (rc != CLY_OK) goto done;
    }
    *n_out = nrec;
    if (nrec > cap) { rc = CLY_ERR_CAPACITY; goto done; }
    if (nrec) {
        CLY_CKG(hipMemcpyAsync(out, d_tup + first, sizeof(cly_tuple) * nrec, hipMemcpyDeviceToHost, st));
        CLY_CKG(hipMemcpyAsync(pos, d_pos, sizeof(cly_pos) * nrec, hipMemcpyDeviceToHost, st));
        CLY_CKG(hipStreamSynchronize(st));
    }
done:
    hipStreamSynchronize(st);
    hipFree(d_bytes); hipFree(d_tup); hipFree(d_pos);
    return rc;
}

// ===========================================================================
// Batched append (the write path: db.appendLogRecord over a batch,
// db.go:368-413, as WriteBatch.Commit issues it, batch.go:62-118): each
// record's Key = encodeKeyWithTxId(key, txId) (batch.go:120-127; db.Put uses
// NO_TX_ID), EncodeLogRecord (data/logRecord.go:57-84), the file rotation
// continuing the active file at its WriteOff, and optionally WriteBatch's
// commit marker {encodeKeyWithTxId(TX_COMMIT_KEY, txId), TxnCommit}.
// Per record two copy descriptors: [header, txId varint, key] and [value].
#define A_PRE 48                                   // header (<= 26) + txId varint (<= 10)
#define A_CMAX 1024                                // descriptors starting in one 4-KiB block
#define A_SMALL_MIN 24                             // smallest record for the A_CMAX / 2 instance of k_mcopy
struct ARec {                                      // == cly_rec_in
    const uint8_t* key;
    const uint8_t* value;
    uint32_t key_len, value_len;
    int64_t expiration;
    uint8_t type, data_type, _pad[6];
};
static_assert(sizeof(ARec) == 40, "cly_rec_in layout");
__device__ const uint8_t g_commit_key = 0x04;      // public.TX_COMMIT_KEY

__device__ __forceinline__ ARec a_rec(const ARec* recs, uint64_t n, uint64_t j) {
    if (j < n) return recs[j];
    ARec c;                                        // the commit marker
    c.key = &g_commit_key; c.value = nullptr; c.key_len = 1; c.value_len = 0; c.expiration = 0;
    c.type = 2; c.data_type = 0;
    return c;
}
__device__ __forceinline__ int a_prefix(const ARec& r, int64_t tx, uint8_t* h) {
    const int tl = uvlen(zz(tx));
    h[4] = r.type;
    h[5] = r.data_type;
    int n = 6;
    n += put_uv(h + n, zz((int64_t)r.key_len + tl));
    n += put_uv(h + n, zz((int64_t)r.value_len));
    n += put_uv(h + n, zz(r.expiration));
    n += put_uv(h + n, zz(tx));
    return n;                                      // header + txId varint
}
__global__ void __launch_bounds__(256)
k_asize(const ARec* __restrict__ recs, uint64_t n, uint64_t nt, int64_t tx, uint64_t* sz, unsigned long long* mx) {
    unsigned long long m = 0, mn = ~0ull;           // largest and smallest encoded record: mx[0], mx[1]
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < nt; j += (uint64_t)gridDim.x * 256) {
        const ARec r = a_rec(recs, n, j);
        uint8_t h[A_PRE];
        sz[j] = (uint64_t)a_prefix(r, tx, h) + r.key_len + r.value_len;
        m = sz[j] > m ? sz[j] : m;
        mn = sz[j] < mn ? sz[j] : mn;
    }
    if (m) atomicMax(mx, m);
    if (mn != ~0ull) atomicMin(mx + 1, mn);
}
// appendLogRecord's rotation from (active file, WriteOff): region 0 is the
// active file (it may take no record), later regions are fresh files that
// always take their first record (a record larger than DataFileSize alone).
__global__ void __launch_bounds__(M_ROT)
k_arot(const uint64_t* __restrict__ g, uint64_t nt, uint64_t total, uint64_t dfs, uint64_t woff, uint32_t max_files,
       uint64_t* fstart, uint64_t* flen, uint32_t* n_out) {
    __shared__ uint64_t s_lo, s_hi;
    uint64_t r = 0;
    uint32_t k = 0;
    while (r < nt || k == 0) {
        const uint64_t g0 = r < nt ? g[r] : total;
        const uint64_t cap = k == 0 ? (woff < dfs ? dfs - woff : 0) : dfs;
        const uint64_t lim = g0 + cap;
        uint64_t lo = k == 0 ? r : r + 1;
        uint64_t hi = r + cap / 9 + 2;
        if (hi > nt) hi = nt;
        if (hi < lo) hi = lo;
        while (lo < hi) {
            const uint64_t span = hi - lo;
            const uint64_t pos = lo + (span * (threadIdx.x + 1) + M_ROT - 1) / M_ROT;
            const int ok = (pos < nt ? g[pos] : total) <= lim;
            const int c = __syncthreads_count(ok);
            if (threadIdx.x == (unsigned)c - 1) s_lo = pos;
            if (threadIdx.x == (unsigned)c) s_hi = pos - 1;
            if (threadIdx.x == 0) { if (c == 0) s_lo = lo; if (c == M_ROT) s_hi = hi; }
            __syncthreads();
            lo = s_lo; hi = s_hi;
            __syncthreads();
        }
        if (threadIdx.x == 0 && k < max_files) {
            fstart[k] = r;
            flen[k] = (k == 0 ? woff : 0) + ((lo < nt ? g[lo] : total) - g0);
        }
        r = lo;
        k++;
        if (r >= nt) break;
    }
    if (threadIdx.x == 0) {
        if (k < max_files) fstart[k] = nt;
        *n_out = k;
    }
}
// per record: region, offset, LogPos, prefix with the CRC, copy descriptors, block map
__global__ void __launch_bounds__(256)
k_aplace(const ARec* __restrict__ recs, uint64_t n, uint64_t nt, int64_t tx, const uint64_t* __restrict__ g,
         const uint64_t* __restrict__ fstart, const uint32_t* __restrict__ n_out_p, uint64_t woff, uint32_t fid0,
         uint64_t stride, MCopy* cp, uint8_t* pre, uint32_t* bmap, cly_pos* pos) {
    __shared__ uint32_t tab[1024];
    crc_table4_init(tab);
    const uint32_t nout = *n_out_p;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < nt; j += (uint64_t)gridDim.x * 256) {
        int lo = 0, hi = (int)nout - 1;                        // region: largest k with fstart[k] <= j
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (fstart[mid] <= j) lo = mid; else hi = mid - 1;
        }
        // region 0 may be empty (fstart[0] == fstart[1] == 0): take the last region starting at or before j
        const uint64_t base = lo == 0 ? woff : 0;
        const uint64_t off = base + (g[j] - g[fstart[lo]]);
        const uint64_t dst = (uint64_t)lo * stride + off;
        const ARec r = a_rec(recs, n, j);
        uint8_t h[A_PRE];
        const int np = a_prefix(r, tx, h);
        uint32_t s = 0xFFFFFFFFu;
        for (int q = 4; q < np; q++) s = crc_upd(tab, s, h[q]);
        s = crc_span(tab, s, r.key, r.key_len);
        s = crc_span(tab, s, r.value, r.value_len);
        s = ~s;
        h[0] = (uint8_t)s; h[1] = (uint8_t)(s >> 8); h[2] = (uint8_t)(s >> 16); h[3] = (uint8_t)(s >> 24);
        uint8_t* pj = pre + (2 * j) * A_PRE;
        for (int q = 0; q < np; q++) pj[q] = h[q];
        const uint32_t ka = (uint32_t)np + r.key_len;
        cp[2 * j] = MCopy{dst, (uint64_t)r.key, ka, (uint32_t)np};
        cp[2 * j + 1] = MCopy{dst + ka, (uint64_t)r.value, r.value_len, 0};
        const uint64_t size = (uint64_t)ka + r.value_len;
        for (uint64_t b = (dst + M_CB - 1) / M_CB; b * M_CB < dst + ka; b++) bmap[b] = (uint32_t)(2 * j);
        for (uint64_t b = (dst + ka + M_CB - 1) / M_CB; b * M_CB < dst + size; b++) bmap[b] = (uint32_t)(2 * j + 1);
        if (j == fstart[0] && lo == 0 && woff % M_CB) bmap[woff / M_CB] = (uint32_t)(2 * j);   // the block WriteOff starts in
        pos[j] = cly_pos{(int64_t)off, fid0 + (uint32_t)lo, 0};
    }
}

__global__ void k_dscale(uint64_t* fstart, uint32_t m) {
    for (uint32_t k = threadIdx.x; k < m; k += blockDim.x) fstart[k] *= 2;
}

extern "C" int cly_append_device(cly_ctx* ctx, const cly_rec_in* d_recs, uint64_t n, int64_t tx_id, int commit,
                                 uint32_t active_fid, uint64_t write_off, uint64_t data_file_size, uint8_t* d_out,
                                 uint32_t out_max_files, uint64_t* out_file_len, cly_pos* d_pos,
                                 cly_append_result* ar, void* stream_v) {
    if (!ctx || !ar || (n && !d_recs) || data_file_size == 0) return CLY_ERR_ARG;
    memset(ar, 0, sizeof(*ar));
    // regions are DataFileSize apart, or further when a record is larger (the
    // reference writes such a record alone into a fresh file)
    uint64_t stride = (data_file_size + M_CB - 1) / M_CB * M_CB;
    ar->out_stride = stride;
    const uint64_t nt = n + (commit ? 1 : 0);
    if (nt == 0) { ar->n_out_files = 1; ar->final_fid = active_fid; ar->final_write_off = write_off; return CLY_OK; }
    if (2 * nt >= (1ull << 32)) return CLY_ERR_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return CLY_ERR_DEVICE;
    hipStream_t st = stream_v ? (hipStream_t)stream_v : ctx->stream;
    int rc = CLY_OK;
    uint64_t *d_sz = nullptr, *d_g = nullptr, *d_fstart = nullptr, *d_flen = nullptr, *h_flen = nullptr;
    uint32_t *d_nout = nullptr, *d_bmap = nullptr;
    MCopy* d_cp = nullptr;
    uint8_t* d_pre = nullptr;
    void* d_tmp = nullptr;
    size_t tb = 0;
    uint32_t h_nout = 0;
    uint64_t total = 0, last = 0, fcap = 0, nblocks = 0;
    unsigned long long* d_mx = nullptr;
    unsigned long long h_mx = 0, h_mn = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const unsigned grid = (unsigned)((nt + 255) / 256 < 16384 ? (nt + 255) / 256 : 16384);
    CLY_CKG(hipEventCreateWithFlags(&e0, hipEventDisableSystemFence));     // (timing only)
    CLY_CKG(hipEventCreateWithFlags(&e1, hipEventDisableSystemFence));
    CLY_CKG(cly_scratch(ctx, AS_SZ, sizeof(uint64_t) * nt, &d_sz));
    CLY_CKG(cly_scratch(ctx, AS_G, sizeof(uint64_t) * nt, &d_g));
    CLY_CKG(cly_scratch(ctx, AS_NOUT, sizeof(uint32_t), &d_nout));
    CLY_CKG(cly_scratch(ctx, AS_MX, 2 * sizeof(unsigned long long), &d_mx));
    CLY_CKG(hipMemsetAsync(d_mx, 0, sizeof(unsigned long long), st));
    CLY_CKG(hipMemsetAsync(d_mx + 1, 0xff, sizeof(unsigned long long), st));
    CLY_CKG(rocprim::exclusive_scan(nullptr, tb, d_sz, d_g, (uint64_t)0, (size_t)nt, rocprim::plus<uint64_t>(), st));
    CLY_CKG(cly_scratch(ctx, AS_TMP, tb + 16, (char**)&d_tmp));
    CLY_CKG(hipEventRecord(e0, st));
    k_asize<<<grid, 256, 0, st>>>((const ARec*)d_recs, n, nt, tx_id, d_sz, d_mx);
    CLY_CKG(rocprim::exclusive_scan(d_tmp, tb, d_sz, d_g, (uint64_t)0, (size_t)nt, rocprim::plus<uint64_t>(), st));
    CLY_CKG(hipMemcpyAsync(&last, d_sz + nt - 1, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    CLY_CKG(hipMemcpyAsync(&total, d_g + nt - 1, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    CLY_CKG(hipMemcpyAsync(&h_mx, d_mx, sizeof(h_mx), hipMemcpyDeviceToHost, st));
    CLY_CKG(hipMemcpyAsync(&h_mn, d_mx + 1, sizeof(h_mn), hipMemcpyDeviceToHost, st));
    CLY_CKG(hipStreamSynchronize(st));
    total += last;
    {
        // a region holds at most max(DataFileSize, one record, the active file's
        // WriteOff): records beyond a full file start a new one
        uint64_t need = data_file_size;
        if (h_mx > need) need = h_mx;
        if (write_off > need) need = write_off;
        stride = (need + M_CB - 1) / M_CB * M_CB;
        ar->out_stride = stride;
    }
    // two neighbouring regions hold more than DataFileSize bytes (the second
    // exists because the first could not take its first record)
    fcap = 2 * (total + write_off) / data_file_size + 4;
    if (fcap > nt + 2) fcap = nt + 2;
    CLY_CKG(cly_scratch(ctx, AS_FSTART, sizeof(uint64_t) * (fcap + 1), &d_fstart));
    CLY_CKG(cly_scratch(ctx, AS_FLEN, sizeof(uint64_t) * (fcap + 1), &d_flen));
    k_arot<<<1, M_ROT, 0, st>>>(d_g, nt, total, data_file_size, write_off, (uint32_t)fcap, d_fstart, d_flen, d_nout);
    CLY_CKG(hipMemcpyAsync(&h_nout, d_nout, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CLY_CKG(hipStreamSynchronize(st));
    ar->n_out_files = h_nout;
    ar->bytes = total;
    if (h_nout > out_max_files || !d_out || !d_pos) { rc = CLY_ERR_CAPACITY; goto done; }
    nblocks = (uint64_t)h_nout * (stride / M_CB);
    CLY_CKG(cly_scratch(ctx, AS_CP, sizeof(MCopy) * 2 * nt, &d_cp));
    CLY_CKG(cly_scratch(ctx, AS_PRE, (size_t)A_PRE * 2 * nt, &d_pre));
    CLY_CKG(cly_scratch(ctx, AS_BMAP, sizeof(uint32_t) * (nblocks + 1), &d_bmap));
    k_aplace<<<grid, 256, 0, st>>>((const ARec*)d_recs, n, nt, tx_id, d_g, d_fstart, d_nout, write_off, active_fid,
                                   stride, d_cp, d_pre, d_bmap, d_pos);
    {
        // k_mcopy's per-region first descriptor: 2 x the first record
        k_dscale<<<1, 64, 0, st>>>(d_fstart, h_nout + 1);
        const uint64_t wgs = (nblocks + MC_W - 1) / MC_W;
        const unsigned cg = wgs < 16384 ? (unsigned)wgs : 16384u;
        // records of >= A_SMALL_MIN bytes start at most 2 (4096 / 24 + 1) + 2 descriptors in a block:
        // the 512-entry instance (half the LDS: 4 waves/SIMD instead of 2)
        if (h_mn >= A_SMALL_MIN)
            k_mcopy<A_CMAX / 2, A_PRE, false><<<cg, 64 * MC_W, 0, st>>>(d_cp, d_pre, d_bmap, d_fstart, d_flen, stride,
                                                                     nblocks, d_out, write_off, nullptr);
        else
            k_mcopy<A_CMAX, A_PRE, false><<<cg, 64 * MC_W, 0, st>>>(d_cp, d_pre, d_bmap, d_fstart, d_flen, stride,
                                                                 nblocks, d_out, write_off, nullptr);
    }
    CLY_CKG(hipGetLastError());
    CLY_CKG(hipEventRecord(e1, st));
    h_flen = (uint64_t*)malloc(sizeof(uint64_t) * h_nout);
    CLY_CKG(hipMemcpyAsync(h_flen, d_flen, sizeof(uint64_t) * h_nout, hipMemcpyDeviceToHost, st));
    CLY_CKG(hipStreamSynchronize(st));
    for (uint32_t k = 0; k < h_nout; k++) if (out_file_len) out_file_len[k] = h_flen[k];
    ar->final_fid = active_fid + h_nout - 1;
    ar->final_write_off = h_flen[h_nout - 1];
    {
        float ms = 0;
        CLY_CKG(hipEventElapsedTime(&ms, e0, e1));
        ar->append_ms = ms;
    }
done:
    hipStreamSynchronize(st);                     // (the buffers stay in the context's scratch)
    free(h_flen);
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    return rc;
}

// Host-memory entry (the cgo path of the write side): records whose key and
// value point into host memory; the encoded bytes come back per region (region
// 0 from write_off on: out + write_off .. out + out_file_len[0]), positions in
// pos[n (+1)].  A query call (out = NULL) returns the region count and stride.
extern "C" int cly_append(cly_ctx* ctx, const cly_rec_in* recs, uint64_t n, int64_t tx_id, int commit,
                          uint32_t active_fid, uint64_t write_off, uint64_t data_file_size, uint8_t* out,
                          uint32_t out_max_files, uint64_t* out_file_len, cly_pos* pos, cly_append_result* ar) {
    if (!ctx || !ar || (n && !recs) || data_file_size == 0) return CLY_ERR_ARG;
    memset(ar, 0, sizeof(*ar));
    if (hipSetDevice(ctx->device) != hipSuccess) return CLY_ERR_DEVICE;
    hipStream_t st = ctx->stream;
    int rc = CLY_OK;
    uint64_t blob = 0;
    for (uint64_t i = 0; i < n; i++) blob += recs[i].key_len + recs[i].value_len;
    uint8_t* h_blob = (uint8_t*)malloc(blob + 16);
    cly_rec_in* h_recs = (cly_rec_in*)malloc(sizeof(cly_rec_in) * (n + 1));
    uint8_t *d_blob = nullptr, *d_out = nullptr;
    cly_rec_in* d_recs = nullptr;
    cly_pos* d_pos = nullptr;
    uint64_t o = 0;
    const uint64_t nt = n + (commit ? 1 : 0);
    cly_append_result q;
    CLY_CKG(hipMalloc((void**)&d_blob, blob + 16));
    for (uint64_t i = 0; i < n; i++) {
        h_recs[i] = recs[i];
        if (recs[i].key_len) memcpy(h_blob + o, recs[i].key, recs[i].key_len);
        h_recs[i].key = d_blob + o;
        o += recs[i].key_len;
        if (recs[i].value_len) memcpy(h_blob + o, recs[i].value, recs[i].value_len);
        h_recs[i].value = d_blob + o;
        o += recs[i].value_len;
    }
    CLY_CKG(hipMalloc((void**)&d_recs, sizeof(cly_rec_in) * (n + 1)));
    if (blob) CLY_CKG(hipMemcpyAsync(d_blob, h_blob, blob, hipMemcpyHostToDevice, st));
    if (n) CLY_CKG(hipMemcpyAsync(d_recs, h_recs, sizeof(cly_rec_in) * n, hipMemcpyHostToDevice, st));
    rc = cly_append_device(ctx, d_recs, n, tx_id, commit, active_fid, write_off, data_file_size, nullptr, 0, nullptr,
                           nullptr, &q, nullptr);
    *ar = q;
    if (rc != CLY_OK && rc != CLY_ERR_CAPACITY) goto done;
    if (!out || !pos || q.n_out_files > out_max_files) { rc = CLY_ERR_CAPACITY; goto done; }
    CLY_CKG(hipMalloc((void**)&d_out, q.out_stride * q.n_out_files));
    CLY_CKG(hipMalloc((void**)&d_pos, sizeof(cly_pos) * (nt + 1)));
    rc = cly_append_device(ctx, d_recs, n, tx_id, commit, active_fid, write_off, data_file_size, d_out, q.n_out_files,
                           out_file_len, d_pos, ar, nullptr);
    if (rc != CLY_OK) goto done;
    for (uint32_t k = 0; k < ar->n_out_files; k++) {
        const uint64_t from = k == 0 ? write_off : 0;
        if (out_file_len[k] > from)
            CLY_CKG(hipMemcpyAsync(out + k * ar->out_stride + from, d_out + k * ar->out_stride + from,
                                   out_file_len[k] - from, hipMemcpyDeviceToHost, st));
    }
    if (nt) CLY_CKG(hipMemcpyAsync(pos, d_pos, sizeof(cly_pos) * nt, hipMemcpyDeviceToHost, st));
    CLY_CKG(hipStreamSynchronize(st));
done:
    hipStreamSynchronize(st);
    hipFree(d_blob); hipFree(d_recs); hipFree(d_out); hipFree(d_pos);
    free(h_blob); free(h_recs);
    return rc;
}
