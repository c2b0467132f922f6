// clyctx.hip — the context of libclyscan.so (include/clyscan.h: cly_ctx_create,
// cly_ctx_destroy, cly_ctx_set_clock), its scratch arena and cly_strerror.
// Host code only.  The scan's own state hangs off the context and is built
// and released by clyscan.hip (cly_scan_state_*_internal).
#include <stdlib.h>

#include "../../include/clyload.h"
#define CLY_TAG "clyctx"
#include "cly_internal.h"

extern "C" int cly_ctx_create(int device, cly_ctx** out) {
    if (!out) return CLY_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return CLY_ERR_DEVICE;
    CLY_CK(hipSetDevice(device));
    cly_ctx* c = (cly_ctx*)calloc(1, sizeof(cly_ctx));
    if (!c) return CLY_ERR_DEVICE;
    c->device = device;
    int rc = CLY_OK;
    CLY_CKG(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    rc = cly_scan_state_create_internal(device, &c->scan);
done:
    if (rc != CLY_OK) { cly_ctx_destroy(c); return rc; }
    *out = c;
    return CLY_OK;
}

// (also the tear-down of a half-built context: every member may still be null)
extern "C" void cly_ctx_destroy(cly_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    cly_scan_state_destroy_internal(c->scan);
    for (int i = 0; i < CLY_NSLOT; i++) if (c->arena.p[i]) hipFree(c->arena.p[i]);
    if (c->stream) hipStreamDestroy(c->stream);
    free(c);
}

extern "C" void cly_ctx_set_clock(cly_ctx* c, int64_t now_ns) { if (c) c->now_ns = now_ns; }

extern "C" hipError_t cly_scratch_internal(cly_ctx* c, cly_slot slot, size_t bytes, void** out) {
    cly_arena* m = &c->arena;
    if (bytes == 0) bytes = 16;
    if (m->cap[slot] < bytes) {
        if (m->p[slot]) { hipError_t e = hipFree(m->p[slot]); if (e != hipSuccess) return e; }
        m->p[slot] = nullptr;
        m->cap[slot] = 0;
        // 1/8 slack against regrowth; CLY_MERGE_EXACT=1 allocates exactly (the
        // regression test of the round-1 k_mplan fault runs both)
        static const bool exact = getenv("CLY_MERGE_EXACT") != nullptr;
        const size_t want = exact ? bytes : bytes + bytes / 8;
        hipError_t e = hipMalloc(&m->p[slot], want);
        if (e != hipSuccess) return e;
        m->cap[slot] = want;
    }
    *out = m->p[slot];
    return hipSuccess;
}

extern "C" const char* cly_strerror(int code) {
    switch (code) {
        case CLY_END_EOF: return "ok / io.EOF";
        case CLY_END_ZERO: return "io.EOF (zero header)";
        case CLY_END_TORN: return "io.EOF (torn record)";
        case CLY_ERR_CRC: return "invalid crc value, logRecord maybe corrupted";
        case CLY_ERR_TRUNC5: return "5-byte tail: header decode index out of range";
        case CLY_ERR_VARINT: return "varint overflow: header slice bounds out of range";
        case CLY_ERR_OFFSET: return "mmap: invalid ReadAt offset";
        case CLY_ERR_CAPACITY: return "output capacity too small";
        case CLY_ERR_DEVICE: return "HIP device error";
        case CLY_ERR_ARG: return "invalid argument";
        case CLY_ERR_NOREPAIR: return "internal: chain resolution failed";
        case CLY_ERR_DIR: return "the data dir maybe contaminated or damaged";
        case CLY_ERR_MERGE_FIN: return "merge-finished: no readable record / value not an integer";
        case CLY_ERR_KEY_EMPTY: return "the key can not be empty";
        default: return "unknown status";
    }
}
