/*
 * clyread.h — batched ReadLogRecord by position on an AMD Instinct MI355X.
 *
 * Reference interface replaced (paths relative to the CouloyDB tree):
 *   func (db *DB) getLogRecordByPos(pos *data.LogPos) (*data.LogRecord, error)
 *       db.go:676-704, behind Get, HGet, every iterator Value() (iterator.go)
 *       and getNonMergeFileId; one DataFile.ReadLogRecord(pos.Offset)
 *       (data/dataFile.go:64-111) on the file pos.Fid names.
 *
 * One call reads n positions: per position the header decode, the bounds
 * checks and the CRC comparison of ReadLogRecord, and for the records that
 * pass, their value bytes packed back to back.  A position is untrusted input
 * (hint files carry arbitrary (fid, offset) pairs): nothing outside
 * [base, base+len) of a file is read, whatever the positions say.
 *
 * A LogRecordDeleted record (tuple.type == 1) is a record: ReadLogRecord
 * returns it, and its status here is CLY_READ_REC.  getLogRecordByPos's
 * mapping of a tombstone to ErrKeyNotFound (db.go:697-699) is the caller's, by
 * tuple.type.
 *
 * Threading and ownership as in clyscan.h: calls on one context are serialised
 * by the caller; every buffer is caller-owned; nothing is retained.
 */
#ifndef CLYREAD_H
#define CLYREAD_H

#include "clyscan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-position status (int32): a terminal status of ReadLogRecord at that offset
 * (CLY_END_EOF/ZERO/TORN, CLY_ERR_CRC/TRUNC5/VARINT/OFFSET, values as in clyscan.h), or: */
#define CLY_READ_REC     100   /* a record was returned (CRC verified)                        */
#define CLY_READ_NOFILE  101   /* pos.fid is not one of `files`: getLogRecordByPos's
                                  dataFile == nil -> ErrKeyNotFound (db.go:680-686)           */

typedef struct cly_read_result {
    uint64_t n_rec;        /* positions with status CLY_READ_REC                         */
    uint64_t n_eof;        /* END_EOF + END_ZERO + END_TORN                              */
    uint64_t n_crc;        /* CLY_ERR_CRC                                                */
    uint64_t n_other;      /* TRUNC5, VARINT, OFFSET                                     */
    uint64_t n_nofile;
    uint64_t value_bytes;  /* sum of value_size over the REC positions = val_off[n]      */
    uint64_t record_bytes; /* sum of size over the REC positions (bytes CRC'd + 4 each)  */
    double   read_ms;      /* device time, HIP events                                    */
} cly_read_result;

/* Device-resident entry.  `files` is a host array whose bases are device
 * memory (len < 2^47 each; a fid listed twice fails with CLY_ERR_ARG; nfiles
 * == 0 is legal); d_pos, d_tuples (may be NULL), d_status, d_val_off (n + 1
 * entries) and d_values are device memory; rr is host memory.
 *
 * Per position i, independent of every other (any order, duplicates allowed):
 *   pos.fid not in files       -> CLY_READ_NOFILE
 *   pos.offset < 0             -> CLY_ERR_OFFSET
 *   otherwise                  -> one ReadLogRecord(pos.offset) on that file.
 * On CLY_READ_REC d_tuples[i] is the tuple cly_scan emits for a record at that
 * offset (fid, tx_id / txid_len with the 0xFF overflow mark included); on any
 * other status it is zero except fid and offset.  d_val_off[0] = 0 and
 * d_val_off[i+1] - d_val_off[i] = value_size for a REC, else 0; the value of
 * REC position i is d_values[d_val_off[i] .. d_val_off[i+1]).
 *
 * Files are addressed with 64-bit arithmetic: the scan's 2-GiB part views do
 * not apply, any record inside a file is read.
 *
 * d_values == NULL is the verify-and-size pass: statuses, tuples, offsets and
 * rr are final, nothing is copied, CLY_OK.  With d_values != NULL and
 * values_cap < rr->value_bytes the call returns CLY_ERR_CAPACITY with
 * everything but d_values filled and no byte of d_values written.  No byte of
 * d_values at or beyond rr->value_bytes is ever written.
 * n == 0 -> CLY_OK, d_val_off[0] = 0.  Null ctx / rr / d_status / d_val_off,
 * or n > 0 with a null d_pos -> CLY_ERR_ARG.
 * `stream` is a hipStream_t passed as void* (NULL = the context's own).       */
int cly_read_device(cly_ctx* ctx, const cly_file* files, int nfiles,
                    const cly_pos* d_pos, uint64_t n,
                    cly_tuple* d_tuples, int32_t* d_status, uint64_t* d_val_off /* n+1 */,
                    uint8_t* d_values, uint64_t values_cap,
                    cly_read_result* rr, void* stream);

/* Host-memory entry (the cgo path): everything is host memory.  Only the files
 * that at least one position names are copied to the device; then the device
 * entry runs and the results are copied back.  values == NULL is the size
 * pass.                                                                       */
int cly_read(cly_ctx* ctx, const cly_file* files, int nfiles,
             const cly_pos* pos, uint64_t n,
             cly_tuple* tuples, int32_t* status, uint64_t* val_off,
             uint8_t* values, uint64_t values_cap, cly_read_result* rr);

#ifdef __cplusplus
}
#endif
#endif /* CLYREAD_H */
