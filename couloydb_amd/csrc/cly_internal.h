// cly_internal.h — the private, host-side interface between the translation
// units of libclyscan.so: the context, its scratch arena, the two error-check
// macros and every function one .hip file calls in another.  Host code only;
// nothing here is part of the C-ABI in include/.
//
// A file defines CLY_TAG (its name in error messages) before including this.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <time.h>

#include "../../include/clyscan.h"

#ifndef CLY_TAG
#error "define CLY_TAG before including cly_internal.h"
#endif
// A failed HIP call is reported and becomes CLY_ERR_DEVICE: CLY_CK returns it,
// CLY_CKG sets `rc` and jumps to the function's `done:` clean-up label.
#define CLY_CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    fprintf(stderr, CLY_TAG ": %s failed: %s\n", #x, hipGetErrorString(e_)); return CLY_ERR_DEVICE; } } while (0)
#define CLY_CKG(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    fprintf(stderr, CLY_TAG ": %s failed: %s\n", #x, hipGetErrorString(e_)); rc = CLY_ERR_DEVICE; goto done; } } while (0)

// The scratch arena's slots, one per device buffer, named after the buffer.
// An entry point owns its group; a slot is shared only where noted.
enum cly_slot {
    // cly_merge_device (MS_TOT also holds cly_hint_positions_device's counter: no call runs both)
    MS_FB, MS_TOT, MS_PLAN, MS_BSUM, MS_ENT, MS_FSTART, MS_FLEN, MS_CP, MS_PRE, MS_BMAP, MS_HSZ, MS_KEYS, MS_PK, MS_PKC,
    // cly_append_device
    AS_SZ, AS_G, AS_NOUT, AS_MX, AS_TMP, AS_FSTART, AS_FLEN, AS_CP, AS_PRE, AS_BMAP,
    // cly_index_device.  IS_HASH is shared on purpose: the open (clyload.hip) reads the key
    // hashes the last cly_index_device call of the context left there.
    IS_FB, IS_TOT, IS_NSEL, IS_CLS, IS_FLAG, IS_COLL, IS_DEL, IS_APFLAG, IS_KSIG, IS_TXKEY, IS_K2, IS_ORDER, IS_HASH,
    IS_SEL, IS_SIDX, IS_REV, IS_NXT, IS_G, IS_G2, IS_TMP, IS_PK,
    // cly_read_device (RS_H_*: cly_read's staging of the host-memory call)
    RS_TAB, RS_FILES, RS_SPAN, RS_CNT, RS_POFS, RS_MULTI, RS_TOT, RS_SLOT, RS_TMP,
    RS_H_BYTES, RS_H_POS, RS_H_TUP, RS_H_STATUS, RS_H_VOFF, RS_H_VAL,
    CLY_NSLOT
};
struct cly_arena { void* p[CLY_NSLOT]; size_t cap[CLY_NSLOT]; };

struct cly_scan_state;           // the scan's buffers, grids, events and timers (clyscan.hip)
struct cly_ctx {
    int device;
    hipStream_t stream;
    int64_t now_ns;              // loadIndex's time.Now() for the TTL sweep (0: the wall clock per call)
    cly_arena arena;             // grow-only device buffers of merge, append, index and read
    cly_scan_state* scan;
};

static inline int64_t cly_now_ns(const cly_ctx* c) {
    if (c->now_ns) return c->now_ns;
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    return (int64_t)ts.tv_sec * 1000000000ll + ts.tv_nsec;
}

extern "C" {
// clyctx.hip: slot `slot` grown to at least `bytes` (plain hipMalloc, so a warm
// context allocates nothing inside a timed call)
hipError_t cly_scratch_internal(cly_ctx* c, cly_slot slot, size_t bytes, void** out);
// clyscan.hip: the scan-private part of a context (cly_ctx_create / cly_ctx_destroy own the rest)
int cly_scan_state_create_internal(int device, cly_scan_state** out);
void cly_scan_state_destroy_internal(cly_scan_state* s);
// clyscan.hip, the open's scan: the tuple buffer sized by the exact record
// count (*d_out, *cap slots; the caller frees it)
int cly_scan_device_alloc_internal(cly_ctx* c, const cly_file* files, int nfiles, cly_tuple** d_out, uint64_t* cap,
                                   uint64_t* file_first, cly_file_result* res, uint64_t* needed);
// clyorder.hip
int cly_order_keys_internal(hipStream_t st, const cly_tuple* d_tup, uint64_t n, const uint8_t* d_state, uint32_t dt,
                            const uint64_t* first, const uint64_t* bases, int nf, uint32_t** d_ord_out,
                            uint64_t* m_out, uint32_t* rounds_out);
// clyindex.hip: the mask of the key hashes in IS_HASH for n records
uint64_t cly_ix_hash_mask_internal(uint64_t n);
}

template <class T>
static inline hipError_t cly_scratch(cly_ctx* c, cly_slot slot, size_t bytes, T** out) {
    return cly_scratch_internal(c, slot, bytes, (void**)out);
}
