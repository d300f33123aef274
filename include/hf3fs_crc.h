/*
 * hf3fs_crc.h -- C ABI of the MI355X chunk-integrity engine (libhf3fs_crc.so).
 *
 * Drop-in boundary for 3FS's ChecksumInfo path.  Every value
 * is the RAW folly register (no final xor) unless the name ends in _fin, as in
 * the reference: ChecksumInfo.value == folly::crc32c(data, n, ~0U)
 * (src/fbs/storage/Common.h:146-177) and the formatter prints ~value (:771).
 *
 * Conventions
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default
 *     stream of the current device).  Batched calls are asynchronous on it and
 *     never retain caller pointers after the stream work completes.
 *   - d_* arguments are device-accessible addresses (hipMalloc'd HBM, or
 *     hipHostRegister'ed / hipHostMalloc'ed host memory mapped to the device);
 *     h_* arguments are plain host memory.
 *   - The calls operate on the current HIP device of the calling thread; the
 *     per-device constant tables are built on first use (or hf3fs_crc_init).
 *   - No exceptions cross the ABI; return values are the reference's status
 *     codes.  Thread-safe and re-entrant (tables are immutable after init).
 */
#ifndef HF3FS_CRC_H
#define HF3FS_CRC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* enum class ChecksumType : uint8_t (src/fbs/storage/Common.h:66-70) */
enum { HF3FS_CHECKSUM_NONE = 0, HF3FS_CHECKSUM_CRC32C = 1, HF3FS_CHECKSUM_CRC32 = 2 };

/* enum class UpdateType : uint8_t (src/fbs/storage/Common.h:51-57) */
enum { HF3FS_UPDATE_WRITE = 1, HF3FS_UPDATE_TRUNCATE = 4, HF3FS_UPDATE_EXTEND = 8 };
/* UpdateType::COMMIT (Common.h:57): a commit job of hf3fs_crc_update_versioned and
 * hf3fs_crc_update_engine, valid in those calls only */
enum { HF3FS_UPDATE_COMMIT = 16 };
/* UpdateType::REMOVE (Common.h:51-54): a job of hf3fs_crc_forward_prepare / _complete only; the
 * update entry points keep answering kInvalidArg for it */
enum { HF3FS_UPDATE_REMOVE = 2 };

/* Status codes: the reference's numeric codes (src/common/utils/StatusCodeDetails.h). */
enum {
  HF3FS_CRC_OK = 0,
  HF3FS_CRC_INVALID_ARG = 3,                  /* StatusCode::kInvalidArg (:24) */
  HF3FS_CRC_INVALID_FORMAT = 33,              /* StatusCode::kInvalidFormat (:42) */
  HF3FS_CRC_SERDE_INSUFFICIENT_LENGTH = 40,   /* StatusCode::kSerdeInsufficientLength (:44) */
  HF3FS_CRC_RDMA_NO_BUF = 2019,               /* RPCCode::kRDMANoBuf (:106) */
  HF3FS_CRC_CHUNK_METADATA_NOT_FOUND = 4001,  /* StorageCode::kChunkMetadataNotFound (:151) */
  HF3FS_CRC_CHUNK_METADATA_GET_ERROR = 4002,  /* StorageCode::kChunkMetadataGetError (:152) */
  HF3FS_CRC_CHUNK_NOT_COMMIT = 4004,          /* StorageCode::kChunkNotCommit (:154) */
  HF3FS_CRC_CHUNK_NOT_CLEAN = 4005,           /* StorageCode::kChunkNotClean (:155) */
  HF3FS_CRC_CHUNK_STALE_UPDATE = 4006,        /* StorageCode::kChunkStaleUpdate (:156) */
  HF3FS_CRC_CHUNK_MISSING_UPDATE = 4007,      /* StorageCode::kChunkMissingUpdate (:157) */
  HF3FS_CRC_CHUNK_COMMITTED_UPDATE = 4008,    /* StorageCode::kChunkCommittedUpdate (:158) */
  HF3FS_CRC_CHUNK_READ_FAILED = 4010,         /* StorageCode::kChunkReadFailed (:160) */
  HF3FS_CRC_CHUNK_ADVANCE_UPDATE = 4012,      /* StorageCode::kChunkAdvanceUpdate (:162) */
  HF3FS_CRC_CHUNK_SIZE_MISMATCH = 4015,       /* StorageCode::kChunkSizeMismatch (:165) */
  HF3FS_CRC_CHUNK_STALE_COMMIT = 4023,        /* StorageCode::kChunkStaleCommit (:172) */
  HF3FS_CRC_TARGET_STATE_INVALID = 4032,      /* StorageCode::kTargetStateInvalid (:176) */
  HF3FS_CRC_NO_SUCCESSOR_TARGET = 4033,       /* StorageCode::kNoSuccessorTarget (:177) */
  HF3FS_CRC_CHECKSUM_MISMATCH = 4080,         /* StorageCode::kChecksumMismatch (:186) */
  HF3FS_CRC_CHAIN_VERSION_MISMATCH = 4081,    /* StorageCode::kChainVersionMismatch (:187) */
  HF3FS_CRC_CHUNK_VERSION_MISMATCH = 4082,    /* StorageCode::kChunkVersionMismatch (:188) */
  HF3FS_CRC_CHUNK_NOT_FOUND = 7007,           /* StorageClientCode::kChunkNotFound (:228) */
  HF3FS_CRC_CLIENT_CHECKSUM_MISMATCH = 7015,  /* StorageClientCode::kChecksumMismatch (:236) */
  HF3FS_CRC_DEVICE_ERROR = 9001,              /* HIP runtime failure, or an update IO whose verify the
                                                 self-check contradicted (no reference equivalent) */
  HF3FS_CRC_NOT_APPLIED = 9002                /* no reference equivalent: the IO was not reached (see max_rounds);
                                                 chunk untouched, resubmit it */
};

/* ------------------------------------------------------------------------ */
/* context                                                                   */
/* ------------------------------------------------------------------------ */
int hf3fs_crc_init(int device);            /* optional: build device tables eagerly */
void hf3fs_crc_shutdown(void);             /* free every device context */
const char *hf3fs_crc_last_error(void);    /* thread-local message of the last failure */
const char *hf3fs_crc_version(void);

/* Scratch lifetime.  Batch calls without caller scratch (verify with d_computed ==
 * NULL, update, read results, scrub, frames, file digest) run on device buffers the
 * library owns per (stream, calling thread); they grow to the largest call and are
 * kept until one of these calls (or hf3fs_crc_shutdown).  release_stream: after the
 * stream's queued work, free every thread's buffers of `stream`, its side streams and
 * its update-apply grid hints (call it before destroying a stream the library was used
 * on; no thread may use the stream during the call).  Calls captured into a graph (any of the above, and every ticket counter
 * and balance region of a captured launch) get memory of their own, owned by the
 * graph through one hipUserObject per capture (small requests share 256 KiB slabs of
 * the capture): when the graph and every executable graph instantiated from it are
 * destroyed, the buffers are freed by release_graph_scratch, release_stream, at
 * shutdown (after which no graph captured earlier may be replayed), or by an
 * uncaptured call once 64 MiB await freeing (hipFree waits for the whole device, so
 * no call pays it routinely; that wait also covers a replay still in flight when its
 * executable graph was destroyed).  Other graphs are never affected.  A captured
 * hf3fs_crc_update_batch may be the process's first library call, also in a global-mode capture: what
 * the library creates for itself (the device context's tables, the update-apply hint
 * slab, side streams, scratch) is created in relaxed capture mode and is no graph node.
 * release_graph_scratch also frees buffers no graph could take a reference to.
 * graph_scratch_stats: live captured buffers (and their bytes), and those whose graph
 * is gone and that await the next free; any pointer may be NULL. */
int hf3fs_crc_release_stream(void *stream);
int hf3fs_crc_release_graph_scratch(void);
int hf3fs_crc_graph_scratch_stats(uint64_t *live_buffers, uint64_t *live_bytes, uint64_t *dead_buffers);

/* Tuning and test switches: read once per process from
 * HF3FS_CRC_<NAME> (upper case) at the first call; set_option overrides one for
 * every later call (tests, in-process A/B).  Unknown names or values -> kInvalidArg.
 * Names: nt, seg_kib, static, pipe (auto|0|1), balance, record_direct,
 * update_pipeline (mode|unfused|fused), apply_pieces, apply_min_kib, apply_nt,
 * apply_grid (-1 auto, 0 ticketed, 1 one-shot, 2 one-shot on a small grid), apply_piece_kib
 * (4|8|16), frame_stream (auto|0|1), frame_segw, debug, audit, range_stream, list_runs,
 * prehash_rep (1..8 byte runs per wave for the update pre hash and list_runs batches).
 * Test only, settable through set_option alone (the environment is ignored for them):
 * poison (every library scratch word handed to a call -- verify values, call scratch and
 * the byte-balance region -- is first set to this value, 0 = off) and fault_io (IO
 * fault_io - 1 of every update batch is hashed from a wrong start value, 0 = off: the
 * self-check's end-to-end test).
 * Switches of hf3fs_crc_md5_batch alone, described with the call: md5_sort (0|1) and
 * md5_stage (0|1). */
int hf3fs_crc_set_option(const char *name, const char *value);
int hf3fs_crc_get_option(const char *name, char *out, size_t cap);

/* Self-check record.  Every payload an update batch reports as
 * mismatched is re-hashed by the batch's last kernel with an independent method
 * (per-lane serial slicing, no shared code with the pipeline's hash).  If the
 * re-hash equals the client's checksum, the pipeline's verdict was wrong: the IO
 * gets HF3FS_CRC_DEVICE_ERROR instead (chunk untouched, retry the IO) and the
 * inconsistency is recorded here with what the scratch held at that point. */
enum {
  HF3FS_ANOMALY_PAYLOAD_HASH = 1, /* the pipeline's payload hash != the re-hash == the client checksum */
  HF3FS_ANOMALY_PRE_JOB = 2,      /* the payload job's (address, length) != the IO's */
  HF3FS_ANOMALY_PRE_MAX = 4,      /* the job-length maximum word < the payload length */
  HF3FS_ANOMALY_START_ONLY = 8,   /* the pipeline's hash is the start value alone (it saw no bytes) */
  HF3FS_ANOMALY_RUN_COVER = 16    /* the pre hash's byte runs do not cover the payload exactly once */
};
typedef struct hf3fs_crc_anomaly {
  uint32_t count;      /* inconsistencies since the last reset */
  uint32_t kinds;      /* OR of HF3FS_ANOMALY_* over all of them */
  uint32_t kind;       /* the first one: its HF3FS_ANOMALY_* bits */
  uint32_t pipeline;   /* its batch: 0 three-pass, 1 fused; | mode << 8 */
  uint64_t io;         /* its IO index in the batch */
  uint32_t pipeline_hash, rehash, client_checksum, pre_max;
  uint64_t pre_addr, pre_len, payload, length;
} hf3fs_crc_anomaly;
/* Device-synchronizes, copies device `device`'s record to *out, then zeroes it if reset. */
int hf3fs_crc_anomalies(int device, hf3fs_crc_anomaly *out, int reset);

/* ------------------------------------------------------------------------ */
/* scalar algebra (no data bytes; replaces folly/Rust combine calls)          */
/* ------------------------------------------------------------------------ */
/* folly::crc32c_combine (called at Common.h:191): crc1 * x^(8 len2) ^ crc2.
 * Also equals Rust crc32c::crc32c_combine on finalized values (chunk.rs:229). */
uint32_t hf3fs_crc32c_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);
/* folly::crc32_combine (Common.h:195) */
uint32_t hf3fs_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);
/* crc fed `nbytes` zero bytes, for `type` in {CRC32C, CRC32}. */
uint32_t hf3fs_crc_shift(uint8_t type, uint32_t crc, uint64_t nbytes);
/* ChecksumInfo::combine (Common.h:179-198) on {*type,*value} in place:
 * HF3FS_CRC_CHECKSUM_MISMATCH on a type mismatch (self not NONE), no-op for
 * length 0, copy when self is NONE. */
int hf3fs_checksum_combine(uint8_t *type, uint32_t *value, uint8_t other_type, uint32_t other_value,
                           uint64_t length);

/* ChecksumInfo in serde's binary form (src/common/serde/Serde.h:422-445 over
 * DownwardBytes): a table = varint32 byte length (5), then the fields in
 * declaration order -- type (1 byte), value (4 bytes, little-endian); 6 bytes,
 * as tests/storage/store/TestCommonStruct.cc:46-55 asserts.  Returns 6. */
uint32_t hf3fs_checksum_serialize(uint8_t type, uint32_t value, uint8_t *out6);
/* Inverse (Serde.h:465-512, 683-735): a table shorter than its length prefix or
 * a field cut short -> HF3FS_CRC_SERDE_INSUFFICIENT_LENGTH; fields missing at
 * the table's end keep their defaults ({NONE, 0}); bytes past the known fields
 * are skipped.  *consumed = bytes of the table including its prefix. */
int hf3fs_checksum_deserialize(const void *in, uint64_t n, uint8_t *type, uint32_t *value, uint64_t *consumed);

/* ------------------------------------------------------------------------ */
/* batched create / verify / combine on device-resident bytes                */
/* ------------------------------------------------------------------------ */
/* ChecksumInfo::create(type, buf, len, start) for n buffers (Common.h:146-177).
 * d_bufs[i]/d_lens[i]: device address and byte length of buffer i (any
 * alignment, any length including 0).  d_starts: per-buffer startingChecksum
 * or NULL for ~0U.  max_len >= every d_lens[i] (sizes the task grid).
 * d_out[i] receives the raw value; type NONE writes 0 (create's {NONE,0}). */
int hf3fs_crc_create_batch(uint8_t type, const void *const *d_bufs, const uint64_t *d_lens,
                           const uint32_t *d_starts, uint32_t *d_out, uint64_t n, uint64_t max_len, void *stream);

/* Same for n equal-length buffers at d_base + i*stride (the bulk write path:
 * one launch over a resident batch, BASELINE config 2). */
int hf3fs_crc_create_strided(uint8_t type, const void *d_base, uint64_t stride, uint64_t len, uint64_t n,
                             uint32_t start, uint32_t *d_out, void *stream);

/* Write/read verify (ChunkReplica.cc:193-207, StorageClientImpl.cc:1720-1737,
 * BatchReadJob.cc:43-54): recompute create(type, buf_i, len_i) and compare with
 * d_expected[i].  d_mismatch[i] = 1 on mismatch else 0; *d_mismatch_count is
 * SET to the number of mismatches.  d_computed (n u32, may be NULL) receives
 * the recomputed values; when NULL the library uses a scratch buffer of the
 * calling (stream, thread) pair, so concurrent calls never share it, on one
 * stream or on many (a larger n than any earlier call of that pair grows the
 * buffer after a stream synchronize).  A call captured into a graph uses a
 * buffer owned by that graph instead (scratch lifetime, above). */
int hf3fs_crc_verify_batch(uint8_t type, const void *const *d_bufs, const uint64_t *d_lens,
                           const uint32_t *d_expected, uint8_t *d_mismatch, uint32_t *d_mismatch_count,
                           uint32_t *d_computed, uint64_t n, uint64_t max_len, void *stream);
int hf3fs_crc_verify_strided(uint8_t type, const void *d_base, uint64_t stride, uint64_t len, uint64_t n,
                             const uint32_t *d_expected, uint8_t *d_mismatch, uint32_t *d_mismatch_count,
                             uint32_t *d_computed, void *stream);

/* KVCache read-verify (BASELINE config 5): n blocks addressed into one arena by
 * byte offset.  Same outputs as hf3fs_crc_verify_batch.  Graph-capturable. */
int hf3fs_crc_verify_blocks(uint8_t type, const void *d_arena, const uint64_t *d_offsets, const uint32_t *d_lens,
                            const uint32_t *d_expected, uint8_t *d_mismatch, uint32_t *d_mismatch_count,
                            uint32_t *d_computed, uint64_t n, uint32_t max_len, void *stream);

/* ChecksumInfo::combine element-wise on same-typed values: d_acc[i] =
 * combine(~d_acc[i], d_crc2[i], d_len2[i]) (Common.h:191,195); len2 == 0 leaves
 * d_acc[i] unchanged.  type NONE is a no-op. */
int hf3fs_crc_combine_batch(uint8_t type, uint32_t *d_acc, const uint32_t *d_crc2, const uint64_t *d_len2,
                            uint64_t n, void *stream);

/* The typed digest table of n chunks in the reference's wire form: d_out =
 * n x 6 bytes, element i = hf3fs_checksum_serialize(type, d_values[i]). */
int hf3fs_crc_serialize_batch(uint8_t type, const uint32_t *d_values, uint64_t n, uint8_t *d_out, void *stream);

/* _fin helpers: the chunk engine and the Rust crc32c crate carry FINALIZED
 * values (fin = ~raw, ChunkEngine.cc:42,66; chunk.rs:157,229).  In place
 * raw <-> fin for n device values (the map is its own inverse). */
int hf3fs_crc_finalize_batch(uint32_t *d_values, uint64_t n, void *stream);
/* crc32c::crc32c_combine on finalized values (chunk.rs:229): the same algebra
 * as the raw form, fin(A||B) = fin(A) * x^(8 len2) ^ fin(B). */
uint32_t hf3fs_crc32c_combine_fin(uint32_t fin1, uint32_t fin2, uint64_t len2);

/* ------------------------------------------------------------------------ */
/* chunk checksum maintenance: ChunkReplica::update + updateChecksum          */
/* ------------------------------------------------------------------------ */
/* One UpdateIO applied to one device-resident chunk replica.  Field meanings
 * follow UpdateIO (Common.h:331-345) and ChunkMetadata (Common.h:652-677).   */
typedef struct hf3fs_crc_update_io {
  uint64_t chunk;           /* device address of the chunk bytes (capacity >= max(size, offset+length)) */
  uint64_t payload;         /* device address of the write payload (`length` bytes); 0 for truncate/extend */
  uint32_t offset;          /* UpdateIO.offset */
  uint32_t length;          /* UpdateIO.length (truncate/extend: the target chunk length) */
  uint32_t chunk_size;      /* ChunkMetadata.size before this IO */
  uint8_t update_type;      /* HF3FS_UPDATE_{WRITE,TRUNCATE,EXTEND} */
  uint8_t chunk_checksum_type;  /* ChunkMetadata.checksumType */
  uint8_t write_checksum_type;  /* UpdateIO.checksum.type */
  uint8_t flags;            /* HF3FS_UPDATE_FLAG_* */
  uint32_t chunk_checksum;  /* ChunkMetadata.checksumValue (raw) */
  uint32_t write_checksum;  /* UpdateIO.checksum.value (raw) */
  /* outputs */
  uint32_t out_size;        /* ChunkMetadata.size after this IO */
  uint32_t out_checksum;    /* ChunkMetadata.checksumValue after this IO (raw) */
  uint8_t out_checksum_type;
  uint8_t checksum_case;    /* HF3FS_CKCASE_*: which checksum path the reference takes for this IO (0 = not applied) */
  uint8_t reserved1[2];
  int32_t status;           /* HF3FS_CRC_OK, _CHECKSUM_MISMATCH (payload verify failed: chunk untouched), _INVALID_ARG,
                               _DEVICE_ERROR (the self-check contradicted the verify: chunk untouched, retry) */
} hf3fs_crc_update_io;

/* hf3fs_crc_update_io.checksum_case: the reference's per-update checksum
 * counters, so a caller keeps feeding its metrics.
 * Replica IOs (ChunkReplica::updateChecksum, ChunkReplica.cc:25-28,334-389):
 *   NONE -> storage.chunk_update.checksum_none, REUSE -> _reuse,
 *   COMBINE -> _combine, RECOMPUTE -> _read_chunk (prefix + suffix re-read; the
 *   DELTA mode reports the case the reference takes, whatever it computed).
 * Engine IOs (HF3FS_UPDATE_FLAG_ENGINE, chunk.rs:153,156,188,217,233,273):
 *   REUSE -> checksum_reuse (copy_on_write without read), COMBINE ->
 *   checksum_combine (safe_write padding / direct or indirect append),
 *   RECOMPUTE -> checksum_recalculate (copy_on_write with read, truncate
 *   shorten), NONE -> no counter.  The engine's choice between copy_on_write
 *   and safe_write also depends on the allocated capacity (engine.rs:383-385);
 *   it is taken as the chunk size (max_len), which no write exceeds here. */
enum {
  HF3FS_CKCASE_NONE = 1,
  HF3FS_CKCASE_REUSE = 2,
  HF3FS_CKCASE_COMBINE = 3,
  HF3FS_CKCASE_RECOMPUTE = 4
};

enum {
  HF3FS_UPDATE_MODE_REFERENCE = 0, /* ChunkReplica.cc:356-389: recompute prefix + suffix after the write */
  HF3FS_UPDATE_MODE_DELTA = 1      /* read only the overwritten old bytes: new = old*x^(8 dsize) ^ lin(old^new)*x^(...) */
};

/* hf3fs_crc_update_io.flags */
enum {
  /* Chunk-engine semantics (ChunkEngine::update, src/storage/store/ChunkEngine.cc:15-66, over the Rust
   * engine, chunk_engine/src/core/engine.rs:288-420 and alloc/chunk.rs:89-281): the chunk checksum is
   * always CRC32C and always the CRC of the chunk bytes (an empty chunk is ~0 raw = 0 finalized); a write
   * whose checksum type is not CRC32C is taken "without_checksum" (hashed, not verified).  Values stay
   * raw at this ABI, as at the C++ bridge (finalized = ~raw, ChunkEngine.cc:42,66). */
  HF3FS_UPDATE_FLAG_ENGINE = 1,
  /* A resync write (UpdateIO.isSyncing): the forwarded whole chunk replaces the
   * replica's.  Valid only on a WRITE with offset == 0 -- the one shape resync produces
   * (ReliableForwarding.cc:179-206 reads the whole chunk); at any other offset the engine would write
   * stale thread-buffer bytes and the replica a size smaller than the write's end, so any other use
   * (offset != 0, truncate, extend) is kInvalidArg for that IO.  Honoured by hf3fs_crc_update_batch,
   * _update_ordered and _update_cow_batch alike; records with the bit clear behave as before.
   * Replica IOs: the payload verify is as usual, out_size = length (ChunkReplica.cc:289), and the
   * checksum follows updateChecksum with that size (:334-339,392): a write of type NONE or length 0
   * gives case NONE, value 0 and the write's type, every other REUSE of the write checksum.
   * Engine IOs: out_size = length, the checksum is the payload's CRC32C (verified when the write is
   * typed CRC32C, hashed otherwise), the case REUSE: copy_on_write with skip_read (chunk.rs:112,
   * 152-170; engine.rs:378-386).  Nothing is read from the old chunk in either form, and no byte at
   * or beyond `length` is written (in place: the old bytes there stay, outside the new size). */
  HF3FS_UPDATE_FLAG_SYNCING = 2
};

/* Applies n IOs to n DISTINCT chunks: verify the payload checksum
 * (ChunkReplica.cc:193-207), write it with gap zero-fill (:281-292), and set
 * the new chunk checksum (:319-394).  d_ios is device-accessible and updated in
 * place.  max_len = the chunk size (UpdateIO.chunkSize): offset >= max_len or
 * offset + length > max_len is kInvalidArg (ChunkReplica.cc:139-145).
 * `type` is the checksum type the batch hashes bytes in: a write's checksum
 * type must be NONE or `type`; the chunk's stored type may be any type -- a
 * write whose type differs from the chunk's recomputes the prefix and suffix
 * in the write's type and the chunk takes the write's type (ChunkReplica.cc:
 * 340, 356-392).  A truncate / extend hashes in the chunk's type, so its chunk
 * type must be NONE or `type` (else kInvalidArg for that IO).
 * Modes: REFERENCE recomputes prefix + suffix from the chunk bytes, as the
 * reference does.  DELTA reads only the overwritten old bytes and derives the
 * new value from the stored chunk checksum: identical results whenever the
 * stored checksum matches the chunk bytes (the invariant the reference keeps);
 * if metadata and bytes disagree (corruption, stale metadata) DELTA carries
 * the disagreement forward where REFERENCE re-derives from the bytes.
 * Stream behaviour: asynchronous on `stream`.  The three-pass pipeline (DELTA's
 * default) forks the verdicts' finalize onto a side stream the library keeps per
 * (stream, calling thread) and joins it back before the call's last launch
 * (capturable); its apply launches one workgroup per 8 KiB piece on a grid sized
 * from the pair's previous call (option apply_grid). */
int hf3fs_crc_update_batch(uint8_t type, hf3fs_crc_update_io *d_ios, uint64_t n, uint32_t max_len, int mode,
                           void *stream);
/* Bytes of scratch one hf3fs_crc_update_batch of n IOs in `mode` takes.  Outside
 * a stream capture the call uses a buffer the library keeps per (stream, calling
 * thread), grown with a stream synchronize when a call needs more (make one call
 * of the largest size first where that stall matters); a captured call gets a
 * buffer of its own (hipMalloc in relaxed capture mode, kept for the graph's
 * replays; see hf3fs_crc_release_graph_scratch).  Never the stream-ordered pool.
 * Every word the call reads is written by the call first (checked with option poison).
 * The figure is for the ticketed apply; a call with the one-shot apply adds a piece
 * table of 4 B per 8 KiB piece, n * (max_len / 8 KiB + 4) entries. */
size_t hf3fs_crc_update_scratch_bytes(uint64_t n, int mode);

/* A queue of n IOs in ARRIVAL ORDER whose IOs may share a chunk: equivalent to applying d_ios[0],
 * d_ios[1], ... d_ios[n-1] one at a time, each as a one-IO hf3fs_crc_update_batch with the same
 * type, max_len and mode -- the per-chunk serialisation the reference gets from the chunk lock
 * around ChunkReplica::update (one UpdateWorker job per IO, each starting from the ChunkMetadata the
 * previous one left).  IOs on different chunks run in parallel.
 * Identity: two IOs address the same chunk iff their `chunk` fields are equal.  Chunks of different
 * base addresses whose byte ranges overlap are undefined, as for update_batch; so is a payload
 * that overlaps any chunk of the batch.  An IO with chunk == 0 is a chunk of its own.
 * State hand-over: the first IO of a chunk, in index order, takes chunk_size, chunk_checksum_type
 * and chunk_checksum from its own record.  For every later IO of that chunk these three input
 * fields are ignored and OVERWRITTEN with the state its predecessor left, so the caller reads what
 * each IO started from.  Output fields and status keep their meaning for every IO.  An IO that
 * fails (_CHECKSUM_MISMATCH, _INVALID_ARG, _DEVICE_ERROR) leaves bytes and state untouched and its
 * successor starts from the state the failed IO started from: the reference's behaviour when an
 * update fails under the chunk lock.
 * Depth bound: max_rounds in 1..64 (else kInvalidArg) is the largest number of IOs per chunk one
 * call applies; the caller states it so that the call needs no host readback.  An IO with
 * max_rounds or more earlier IOs on its chunk gets status HF3FS_CRC_NOT_APPLIED, checksum_case 0,
 * and input and output state fields equal to the state after the chunk's last applied IO; its
 * chunk bytes are not touched by it (resubmit it unchanged, with the other IOs of its chunk in the
 * same order).  d_info may be NULL; else two device words SET by the call: [0] the longest chain
 * of the batch (uncapped), [1] the number of NOT_APPLIED IOs.
 * With all chunks distinct the call writes exactly the bytes hf3fs_crc_update_batch writes, into
 * the IO records and into the chunks, under every option; the error returns match too (unknown
 * type or mode, null d_ios with n > 0 -> kInvalidArg, n == 0 -> OK; all checked before any device
 * is touched).
 * Stream behaviour: asynchronous on `stream`, no host synchronisation, nothing read back from the
 * device; capturable, also as the process's first library call.  Ranking happens in kernels: a
 * replayed graph re-plans from what d_ios holds at replay time.  Scratch follows update_batch's
 * lifetime rules (per (stream, thread) outside a capture, graph-owned inside one, never the
 * stream-ordered pool), and every scratch word the call reads it wrote first (option poison).
 * Cost: a hash table of the chunk addresses, then max_rounds passes of the update pipeline over
 * n records of which pass r holds the IOs with r earlier IOs on their chunk (the rest are no-op
 * records), so size max_rounds to the queue, not to 64.  Ranking walks, per IO, the list of its
 * chunk's IOs: O(multiplicity) per IO -- one chunk taking all n IOs costs n^2 list steps. */
int hf3fs_crc_update_ordered(uint8_t type, hf3fs_crc_update_io *d_ios, uint64_t n, uint32_t max_len, int mode,
                             uint32_t max_rounds, uint32_t *d_info, void *stream);
/* Bytes of scratch one such call takes, for the pipeline the options select and including the
 * one-shot apply's piece table for max_len wherever a call of this shape may use it: after one
 * call of the largest (n, max_len, max_rounds) of a mode, no later call on the pair grows the
 * buffer.  0 for arguments the call would reject. */
size_t hf3fs_crc_update_ordered_scratch_bytes(uint64_t n, uint32_t max_len, int mode, uint32_t max_rounds);

/* The version state of one job of hf3fs_crc_update_versioned, parallel to its hf3fs_crc_update_io:
 * what UpdateWorker knows from the UpdateJob (io_ver, job_chain_ver, is_force) and the chunk's
 * ChunkMetadata (Common.h:652-677) before the job, and the metadata the job leaves. */
typedef struct hf3fs_crc_update_ver {
  uint32_t io_ver;          /* UpdateIO.updateVer (0: this replica assigns) / CommitIO.commitVer */
  uint32_t job_chain_ver;   /* job.commitChainVer() */
  /* ChunkMetadata before the job: read from the chunk's first job, OVERWRITTEN for every later one */
  uint32_t chain_ver, update_ver, commit_ver;
  uint32_t meta_chunk_size; /* meta.innerFileId.chunkSize */
  uint8_t chunk_state;      /* HF3FS_CHUNK_STATE_*: COMMIT 0, DIRTY 1, CLEAN 2 */
  uint8_t recycle_state;    /* 0 = NORMAL */
  uint8_t is_force;         /* CommitIO.isForce */
  uint8_t reserved0;
  /* ChunkMetadata after the job (== before, when the job fails) */
  uint32_t out_chain_ver, out_update_ver, out_commit_ver;
  uint8_t out_chunk_state, out_recycle_state, reserved1[2];
  uint32_t reserved2;
} hf3fs_crc_update_ver;

/* enum class ChunkState : uint8_t (Common.h) */
enum { HF3FS_CHUNK_STATE_COMMIT = 0, HF3FS_CHUNK_STATE_DIRTY = 1, HF3FS_CHUNK_STATE_CLEAN = 2 };

/* Words of hf3fs_crc_update_versioned's d_info */
enum {
  HF3FS_VER_INFO_CHAIN_MAX = 0,     /* longest chain of the batch (uncapped) */
  HF3FS_VER_INFO_NOT_APPLIED = 1,   /* NOT_APPLIED jobs */
  HF3FS_VER_INFO_UPDATES = 2,       /* applied updates */
  HF3FS_VER_INFO_COMMITS = 3,       /* applied commits */
  HF3FS_VER_INFO_REFUSED = 4,       /* jobs with any other non-zero status */
  HF3FS_VER_INFO_FATAL = 5,         /* the reference's fatal events among them (4080, 4081, 4082) */
  HF3FS_VER_INFO_COMMIT_DIRTY = 6,  /* commits refused DIRTY (storage.commit.dirty) */
  HF3FS_VER_INFO_COMMIT_STALE = 7,  /* stale commits (storage.commit.stale) */
  HF3FS_VER_INFO_WORDS = 8
};

/* hf3fs_crc_update_ordered with the part of ChunkReplica::update that decides whether a job may run
 * at all: the updateVer / commitVer / chainVer / ChunkState ladder (ChunkReplica.cc:171-191,211-245)
 * and ChunkReplica::commit (:397-467) as a job of the same queue.  n jobs in ARRIVAL ORDER; job i
 * is d_ios[i] with d_ver[i].  Identity, the hand-over of {size, checksum type, checksum value},
 * max_rounds in 1..64, NOT_APPLIED, stream, capture, scratch and poison rules are update_ordered's.
 * With d_ver == NULL the call IS hf3fs_crc_update_ordered, byte for byte, d_info's two words
 * included (HF3FS_UPDATE_COMMIT is then an unknown update type, kInvalidArg for that IO).
 * State hand-over: the chunk's first job takes chain_ver, update_ver, commit_ver, meta_chunk_size,
 * chunk_state and recycle_state from its own record; for every later job these six are OVERWRITTEN
 * with what its predecessor left.  A chunk without metadata (kChunkMetadataNotFound, :154-164) is
 * described by the caller: size 0, versions 0, chunk_state CLEAN, chain_ver = job_chain_ver,
 * meta_chunk_size = max_len.  out_* are the metadata after the job; the IOResult version fields
 * the reference returns (updateVer, commitVer, commitChainVer) are out_* on success and the
 * before-state on failure, which out_* then repeat.
 * An update job (WRITE / TRUNCATE / EXTEND, replica IOs) gets the first status that holds:
 *   1. kInvalidArg: every one the plain call gives for the record; HF3FS_UPDATE_FLAG_ENGINE (the
 *      engine's ladder, engine.rs:340-365, is another one); any other update type (REMOVE).
 *   2. 4015 meta_chunk_size != max_len (:176).
 *   3. 4005 chunk_state DIRTY and the IO is not HF3FS_UPDATE_FLAG_SYNCING (:181).
 *   4. 4081 job_chain_ver < chain_ver and chunk_state COMMIT (:186).
 *   5. 4080 from the payload verify (:193-207); the self-check's 9001 stands here too.
 *   6. Syncing: update_ver = io_ver, commit_ver = io_ver - 1, recycle_state = 0.
 *      io_ver > 0: 4008 if io_ver <= commit_ver; 4006 if io_ver <= update_ver; 4007 if io_ver >
 *      update_ver + 1; else update_ver = io_ver.
 *      io_ver == 0: 4012 if update_ver + 1 > commit_ver + 1; else update_ver += 1.
 *   7. applied exactly as update_ordered applies it; chunk_state CLEAN, chain_ver = job_chain_ver.
 * A payload mismatch wins over a refusal at rung 6; a job refused at rungs 1-4 is never hashed.
 * A commit job (update_type HF3FS_UPDATE_COMMIT; payload, offset, length are ignored) takes one
 * round and touches no byte: kInvalidArg on a chunk with recycle_state != 0 (that commit is
 * store.remove, left to the host) or with the ENGINE flag; 4081 if job_chain_ver < chain_ver; 4082
 * if io_ver > update_ver; is_force: CLEAN, commit_ver = io_ver; else DIRTY -> 4005; else
 * commit_ver < io_ver sets it; else 4023.  Then commit_ver == update_ver makes the chunk COMMIT with
 * chain_ver = job_chain_ver.  Its out_size / out_checksum{,_type} repeat the chunk's, case 0.
 * Every failure leaves bytes, size, checksum and version state untouched; the chunk's next job
 * starts from them.  For a refused job the output fields of d_ios are those of an IO that failed
 * its verify (the input state repeated, case 0) with the refusal in status.  Version arithmetic is
 * uint32_t (ChunkVer).  A NOT_APPLIED job carries the chunk's state after its last applied job in
 * the input and the out_* fields of both records.
 * d_info may be NULL; else HF3FS_VER_INFO_WORDS device words SET by the call.
 * Cost on top of update_ordered: the step between rounds reads and writes the 48-byte records and
 * runs the ladders; after the last round one hashing pass verifies the payloads of the jobs refused
 * at rung 6 (nothing to hash when there is none) and one kernel settles them and counts d_info.
 * Nothing is decided on the host or read back: a replayed graph re-plans from the records. */
int hf3fs_crc_update_versioned(uint8_t type, hf3fs_crc_update_io *d_ios, hf3fs_crc_update_ver *d_ver, uint64_t n,
                               uint32_t max_len, int mode, uint32_t max_rounds, uint32_t *d_info, void *stream);
/* Bytes of scratch one such call with version records takes (update_ordered's rule: after one call
 * of the largest shape nothing grows).  0 for arguments the call would reject. */
size_t hf3fs_crc_update_versioned_scratch_bytes(uint64_t n, uint32_t max_len, int mode, uint32_t max_rounds);

/* The engine state of one job of hf3fs_crc_update_engine, parallel to its hf3fs_crc_update_io: what
 * ChunkEngine::update / ::commit take from the UpdateJob (ChunkEngine.cc:39-40,96), the chunk's
 * committed ChunkMeta and writing-list entry before the job, and what the job leaves.  The committed
 * len and checksum are chunk_size / chunk_checksum_type / chunk_checksum of the IO record. */
typedef struct hf3fs_crc_engine_job {
  uint64_t dst;             /* a fresh allocation (capacity >= max_len) the job may copy_on_write into; 0 = none */
  /* engine state before the job: read from the chunk's first job, OVERWRITTEN for every later one */
  uint64_t addr;            /* device address of the committed version */
  uint64_t w_addr;          /* device address of the writing version; 0 = no live holder */
  /* engine state after the job (== before, when the job fails) */
  uint64_t out_addr;
  uint64_t out_w_addr;
  uint32_t io_ver;          /* UpdateReq.update_ver (0: the engine assigns chunk_ver + 1) */
  uint32_t job_chain_ver;   /* job.commitChainVer() */
  uint32_t chain_ver, chunk_ver;                              /* before: committed ChunkMeta */
  uint32_t w_len, w_checksum, w_chain_ver, w_chunk_ver;       /* before: the writing version (checksum raw) */
  uint32_t out_chain_ver, out_chunk_ver;                      /* after: committed */
  uint32_t out_w_len, out_w_checksum, out_w_chain_ver, out_w_chunk_ver;  /* after: writing */
  uint8_t out_cow;          /* 1: the job wrote into dst */
  uint8_t detail;           /* HF3FS_ENGINE_DETAIL_*: why status is kInvalidArg */
  uint8_t reserved[6];
} hf3fs_crc_engine_job;

/* hf3fs_crc_engine_job.detail */
enum {
  HF3FS_ENGINE_DETAIL_NONE = 0,
  HF3FS_ENGINE_DETAIL_RECORD = 1,      /* malformed record, no ENGINE flag, or an update type the call does not take */
  HF3FS_ENGINE_DETAIL_IN_WRITING = 2,  /* the chunk has a live writing version (engine.rs:441-447) */
  HF3FS_ENGINE_DETAIL_NO_DST = 3,      /* copy-on-write needed and dst == 0 */
  HF3FS_ENGINE_DETAIL_NO_WRITING = 4   /* a commit without a writing version */
};

/* Words of hf3fs_crc_update_engine's d_info */
enum {
  HF3FS_ENGINE_INFO_CHAIN_MAX = 0,    /* longest chain of the batch (uncapped) */
  HF3FS_ENGINE_INFO_NOT_APPLIED = 1,  /* NOT_APPLIED jobs */
  HF3FS_ENGINE_INFO_UPDATES = 2,      /* applied updates */
  HF3FS_ENGINE_INFO_COMMITS = 3,      /* applied commits */
  HF3FS_ENGINE_INFO_REFUSED = 4,      /* jobs with any other non-zero status */
  HF3FS_ENGINE_INFO_COW = 5,          /* applied updates that copied on write (copy_on_write_times) */
  HF3FS_ENGINE_INFO_IN_PLACE = 6,     /* applied updates written in place (safe_write) */
  HF3FS_ENGINE_INFO_IN_WRITING = 7,   /* updates refused because the chunk was in writing */
  HF3FS_ENGINE_INFO_WORDS = 8
};

/* The queue of a chunk-engine target in ARRIVAL ORDER: ChunkEngine::update (ChunkEngine.cc:15-80)
 * over Engine::update_chunk (chunk_engine/src/core/engine.rs:288-468) and ChunkEngine::commit
 * (ChunkEngine.cc:82-110, engine.rs:470-507) as jobs of one call, with nothing decided on the host:
 * the engine's version checks, the writing list, copy_on_write or safe_write chosen from the state
 * each job actually meets, and the committed address moving to the destination at commit.  Job i is
 * d_ios[i] with d_jobs[i].  max_rounds in 1..64, HF3FS_CRC_NOT_APPLIED, stream, capture, scratch and
 * poison rules are hf3fs_crc_update_versioned's.  Argument errors (before any device is touched):
 * those of update_versioned; type must be HF3FS_CHECKSUM_CRC32C (the engine knows no other);
 * d_jobs == NULL with n > 0; a batch whose piece table would pass 1 GiB (as update_cow_batch).
 * Identity: two jobs address the same chunk iff their d_ios[i].chunk are equal.  In this call
 * `chunk` is a key only and is never dereferenced (normally the committed address at queue time);
 * the bytes are found through `addr`.
 * State hand-over: the chunk's first job takes addr, chain_ver, chunk_ver, the five w_* fields and
 * the IO record's chunk_size / chunk_checksum_type / chunk_checksum from its own records; for every
 * later job they are OVERWRITTEN with what its predecessor left.  Unlike update_ordered the next job
 * starts from the COMMITTED {size, checksum}, which an update does not change, and with the writing
 * fields set.  A chunk the engine does not know (engine.rs:327-337) is described by the caller:
 * size 0, chunk_ver 0, chain_ver = job_chain_ver, addr = the allocation the engine would make (:405).
 * An update job (WRITE / TRUNCATE / EXTEND with HF3FS_UPDATE_FLAG_ENGINE) gets the first that holds:
 *   1. kInvalidArg, detail 1: every kInvalidArg the plain call gives for the record; a record
 *      without the ENGINE flag; any other update type (REMOVE stays on the host).
 *   2. 4080 from the payload verify (engine.rs:297-311); the self-check's 9001 stands here too.  It
 *      precedes every version rung: a job refused at 3-6 still has its payload hashed, 4080 wins.
 *   3. 4081 if job_chain_ver < chain_ver (:340).
 *   4. Not syncing and io_ver > 0: 4008 if io_ver <= chunk_ver; 4007 if io_ver > chunk_ver + 1.
 *   5. kInvalidArg, detail 3, if the job must copy on write and dst == 0.
 *   6. kInvalidArg, detail 2, if w_addr != 0 (:441-447).
 *   7. Applied.  The new version is io_ver (syncing, or io_ver > 0), else chunk_ver + 1, in uint32_t
 *      arithmetic (the engine's release build wraps).  Copy on write iff syncing, or a WRITE with
 *      length > 0 && offset < chunk_size (:377-380; the capacity clause never holds: capacity is
 *      taken as max_len): the record is applied exactly as hf3fs_crc_update_cow_batch applies it
 *      from addr into dst, out_cow = 1.  Otherwise it is applied in place at addr exactly as
 *      hf3fs_crc_update_batch does (safe_write) and dst is not touched.  Afterwards the writing
 *      version is {out_cow ? dst : addr, out_size, out_checksum, job_chain_ver, new version}; the
 *      committed state is unchanged.  out_size, out_checksum and checksum_case of the IO record are
 *      the pipeline's: what ChunkEngine::update returns (:61-66).
 * A commit job (update_type HF3FS_UPDATE_COMMIT; payload, offset, length, io_ver ignored) takes one
 * round and touches no byte: kInvalidArg, detail 4, if w_addr == 0; else the committed state becomes
 * the writing version with chain_ver = job_chain_ver and the writing fields are cleared: out_addr =
 * w_addr, out_size / out_checksum repeat the new committed state (type CRC32C), checksum_case 0.
 * The caller recycles the old allocation when out_addr != addr; a dst whose job came back with
 * out_cow == 0 goes back to the allocator.
 * Every failure leaves bytes, committed and writing state untouched; out_* repeat the before-state
 * and the IO record's outputs are those of an IO that failed its verify (input state repeated,
 * case 0).  A NOT_APPLIED job carries the chunk's state after its last applied job in the input and
 * out_* fields of both records.
 * Two deliberate differences from the reference: on 4080 its IOResult carries zero versions
 * (engine.rs:303 returns before :322), this call repeats the before-state like every other refusal;
 * and a job refused "in writing" has, in the reference, already written its bytes (a safe_write
 * scribbles past the committed length at the shared position) -- here a refused job writes nothing.
 * d_info may be NULL; else HF3FS_ENGINE_INFO_WORDS device words SET by the call.
 * Aliasing: every dst has capacity >= max_len and overlaps no chunk, payload, record or other dst
 * of the batch; anything else is undefined, as for update_cow_batch.
 * Pipeline: every round is update_cow_batch's (three passes, one-shot apply) with a per-round
 * destination array; the grid hint word is the call's own, so update_batch, update_ordered,
 * update_versioned and update_cow_batch calls on the same pair plan as if no engine call had run. */
int hf3fs_crc_update_engine(uint8_t type, hf3fs_crc_update_io *d_ios, hf3fs_crc_engine_job *d_jobs, uint64_t n,
                            uint32_t max_len, int mode, uint32_t max_rounds, uint32_t *d_info, void *stream);
/* Bytes of scratch one such call takes (after one call of the largest (n, max_len, max_rounds)
 * nothing grows).  0 for arguments the call would reject. */
size_t hf3fs_crc_update_engine_scratch_bytes(uint64_t n, uint32_t max_len, int mode, uint32_t max_rounds);

/* hf3fs_crc_update_batch with a destination per IO: Chunk::copy_on_write (chunk_engine/src/alloc/
 * chunk.rs:89-174), which writes the new version of a chunk into a newly allocated one and leaves
 * the committed version readable.  d_dst is a device array of n destination addresses, or NULL.
 * In place: d_dst == NULL, d_dst[i] == 0 or d_dst[i] == d_ios[i].chunk applies IO i exactly as
 * hf3fs_crc_update_batch does; with d_dst == NULL the call writes byte for byte what update_batch
 * writes, into the records and into the chunks.  The error returns match too (unknown type or mode,
 * null d_ios with n > 0 -> kInvalidArg, n == 0 -> OK; all checked before any device is touched);
 * one more: a batch whose piece table (below) would pass 1 GiB is kInvalidArg -- split it.
 * Out of place (any other d_dst[i]): for an IO whose status comes back OK, dst[0, out_size) becomes
 * the chunk image the reference leaves -- the old bytes outside the write, the gap zero-fill, the
 * payload, the zero extension of an extend; a shortening truncate copies [0, target).  This holds
 * for every OK IO, also one that changes no byte (a zero-length write, a truncate to the current
 * size).  No byte of `chunk` is written and no byte of dst at or beyond out_size (the engine's
 * 512-byte write padding is not modelled).  An IO that fails (_CHECKSUM_MISMATCH, _INVALID_ARG,
 * _DEVICE_ERROR) leaves chunk and dst untouched.  Every output field and checksum_case have the
 * values the in-place call gives for the same IO, in both modes.  On commit the caller swaps the
 * chunk address for the destination.
 * Aliasing: dst has capacity >= max(chunk_size, offset + length) and overlaps no chunk, payload,
 * record or other destination of the batch; anything else is undefined, as for update_batch.
 * Pipeline: pinned in both modes to the three passes (prep, pre hash, apply) with the one-shot
 * apply: prep emits up to four self-describing range records per IO -- payload, gap, old prefix
 * [0, min(offset, size)), old suffix [min(offset + length, size), size); truncate / extend
 * [0, min(size, new size)) -- and one workgroup copies one piece of one range.  DELTA hashes the old
 * bytes under the write from `chunk`; REFERENCE hashes prefix and suffix from the new image in dst.
 * Options honoured: apply_piece_kib (4|8|16), apply_nt bit 0 (non-temporal loads), apply_grid = 2
 * (one workgroup per CU, each looping over pieces; any other value sizes the grid from the pair's
 * previous COW call, the first call from the CU count), prehash_rep, audit, debug, poison, fault_io.
 * Ignored: update_pipeline, apply_pieces, apply_min_kib, apply_nt bits 1-2, apply_grid = 0 (there
 * is no ticketed form).  The grid hint word is the call's own: plain update_batch calls on the same
 * (stream, thread) pair plan as if no COW call had run.
 * Stream behaviour follows update_batch: asynchronous, capturable (also as the process's first
 * library call), no host readback; scratch per (stream, thread) pair outside a capture and
 * graph-owned inside one, never the stream-ordered pool; every scratch word read is written by the
 * call first (option poison). */
int hf3fs_crc_update_cow_batch(uint8_t type, hf3fs_crc_update_io *d_ios, const uint64_t *d_dst, uint64_t n,
                               uint32_t max_len, int mode, void *stream);
/* Bytes of scratch one such call takes, piece table included: after one call of the largest
 * (n, max_len) nothing grows.  The table holds one 4-byte entry per piece of P = apply_piece_kib
 * bytes.  A range of L bytes at any address has at most floor((L + 2 P - 2) / P) <= L / P + 2
 * pieces, and the (at most four) ranges of an IO are disjoint inside [0, max_len), so an IO takes
 * at most max_len / P + 8 entries: n * (max_len / P + 8) in all.  0 for arguments the call rejects. */
size_t hf3fs_crc_update_cow_scratch_bytes(uint64_t n, uint32_t max_len, int mode);
/* Test aid: *call_bytes = bytes of the calling (stream, thread) pair's call scratch (0: none yet),
 * *allocations = allocations and growths of pair buffers in this process so far; either may be NULL. */
int hf3fs_crc_pair_scratch_stats(void *stream, uint64_t *call_bytes, uint64_t *allocations);

/* ------------------------------------------------------------------------ */
/* read results: AioReadJob::setResult checksum part                          */
/* ------------------------------------------------------------------------ */
/* One completed chunk read (src/storage/aio/BatchReadJob.cc:24-63). */
typedef struct hf3fs_crc_read_io {
  uint64_t data;            /* device address of the read bytes (localbuf + headLength) */
  uint32_t offset;          /* ReadIO.offset */
  uint32_t length;          /* bytes actually read (*lengthInfo) */
  uint32_t chunk_len;       /* state_.chunkLen */
  uint8_t batch_checksum_type;  /* BatchReadReq checksumType */
  uint8_t chunk_checksum_type;  /* state_.chunkChecksum.type */
  uint8_t recalculate;      /* batch_.recalculateChecksum() (resync full-chunk reads) */
  uint8_t reserved0;
  uint32_t chunk_checksum;  /* state_.chunkChecksum.value (raw) */
  /* outputs */
  uint32_t out_checksum;    /* IOResult.checksum.value */
  uint8_t out_checksum_type;
  uint8_t reserved1[3];
  int32_t status;           /* 0, or 4080 when the recalculated full-chunk checksum differs */
  uint32_t reserved2;
} hf3fs_crc_read_io;

/* For n completed reads: NONE batch -> {NONE,0}; a full-chunk read of the
 * stored type reuses the chunk checksum; otherwise the read bytes are hashed;
 * with `recalculate`, full-chunk reads are re-hashed and compared with the
 * stored checksum (status 4080 on mismatch).  Non-NONE types must equal
 * `type`.  max_len >= every length. */
int hf3fs_crc_read_result_batch(uint8_t type, hf3fs_crc_read_io *d_ios, uint64_t n, uint32_t max_len, void *stream);

/* ------------------------------------------------------------------------ */
/* file digest: admin `checksum --fill-zero`                                  */
/* ------------------------------------------------------------------------ */
/* One chunk read of a file, in file order (FileWrapper.cc:133-160). */
typedef struct hf3fs_crc_block_digest {
  uint64_t read_len;        /* *lengthInfo; 0 for kChunkNotFound */
  uint64_t block_len;       /* ReadIO.length (the bytes the file holds there) */
  uint32_t checksum;        /* readIO.result.checksum.value (raw) */
  uint8_t checksum_type;    /* readIO.result.checksum.type; NONE for a missing chunk */
  uint8_t missing;          /* 1: the read failed with kChunkNotFound (read_len and checksum ignored) */
  uint8_t reserved[2];
} hf3fs_crc_block_digest;

/* Digest of one file (or one replica of it). */
typedef struct hf3fs_crc_file_digest {
  uint64_t length;          /* sum of block_len */
  uint32_t value;           /* ChecksumInfo.value (raw) */
  uint8_t type;             /* ChecksumInfo.type */
  uint8_t reserved[3];
  int32_t status;           /* 0; 3 if any block has an unknown type, or (fill-zero) read_len > block_len
                               (checked before the fold); else the first error in file order: 4080 on a
                               type mismatch, and without fill-zero 7007 for a missing chunk, 33 for a
                               read whose length differs from block_len */
  uint32_t reserved2;
} hf3fs_crc_file_digest;

/* FileWrapper::readFile's checksum fold with fillZero (FileWrapper.cc:119-164;
 * called per replica by Checksum.cc:43-88), for n_files files at once: file f
 * owns blocks [d_file_off[f], d_file_off[f+1]) of d_blocks.  Short reads are
 * zero-filled with CRC32C, each block is folded with ChecksumInfo::combine
 * (block, block_len); the result (or the first error's status) goes to
 * d_out[f].  max_blocks >= every file's block count (sizes the grid). */
int hf3fs_crc_file_digest_batch(const hf3fs_crc_block_digest *d_blocks, const uint64_t *d_file_off,
                                hf3fs_crc_file_digest *d_out, uint64_t n_files, uint64_t max_blocks, void *stream);

/* The same fold with the admin command's options (Checksum.cc:43-88 passes --fill-zero to
 * FileWrapper::readFile, FileWrapper.cc:133-160).  HF3FS_DIGEST_FILL_ZERO: as above.
 * Without it, blocks are taken in file order and the first failing one ends the
 * fold: a missing chunk -> HF3FS_CRC_CHUNK_NOT_FOUND (the read error, :134-139), a
 * read of another length than block_len -> HF3FS_CRC_INVALID_FORMAT ("read is
 * short", :153-160), a type mismatch of the combine -> HF3FS_CRC_CHECKSUM_MISMATCH. */
enum { HF3FS_DIGEST_FILL_ZERO = 1 };
int hf3fs_crc_file_digest_batch_ex(const hf3fs_crc_block_digest *d_blocks, const uint64_t *d_file_off,
                                   hf3fs_crc_file_digest *d_out, uint64_t n_files, uint64_t max_blocks,
                                   uint32_t flags, void *stream);

/* ------------------------------------------------------------------------ */
/* client batchRead completion: the verify ladder and the split-read merge    */
/* ------------------------------------------------------------------------ */
/* One ReadIO as StorageClientImpl::batchRead sent it: a split child, or an unsplit IO
 * (src/client/storage/StorageClientImpl.cc:1720-1737 reads these fields). */
typedef struct hf3fs_crc_client_read_io {
  uint64_t data;          /* device address of readIO->data (read with VERIFY only) */
  uint32_t length;        /* ReadIO.length (requested) */
  uint32_t read_len;      /* *result.lengthInfo when status_in == 0 */
  int32_t status_in;      /* 0: lengthInfo holds a value; else result.lengthInfo.error().code() */
  uint32_t checksum;      /* result.checksum.value as the server sent it (raw) */
  uint8_t checksum_type;  /* result.checksum.type */
  uint8_t reserved0[3];
  /* outputs */
  uint32_t computed;      /* the local ChecksumInfo::create value when the IO was hashed, else 0 */
  int32_t status;         /* result after the verify: status_in, 7015 on mismatch, 3 for a bad record */
  uint32_t reserved1;
} hf3fs_crc_client_read_io;

/* parentIO->result after the merge loop (StorageClientImpl.cc:1607-1633). */
typedef struct hf3fs_crc_client_read_result {
  uint32_t length;        /* lengthInfo value (mod 2^32, as the reference sums it, :1629); 0 when status != 0 */
  uint32_t checksum;
  uint8_t checksum_type;
  uint8_t reserved[3];
  int32_t status;         /* 0, or the taking-over child's status; 7003 for a parent without children */
  uint32_t failed_child;  /* index in d_ios of the child that took over, ~0u if none */
  uint32_t block_len;     /* sum of the children's `length` (mod 2^32) */
} hf3fs_crc_client_read_result;

enum { HF3FS_CRC_CLIENT_NOT_INITIALIZED = 7003 }; /* StorageClientCode::kNotInitialized (:224): IOResult's default */
enum { HF3FS_CLIENT_READ_VERIFY = 1 };            /* flags: options.verifyChecksum() (:1720) */
enum {                                            /* words of d_info */
  HF3FS_CLIENT_READ_INFO_BAD_CHILDREN = 0,        /* children whose status after the verify is not 0 */
  HF3FS_CLIENT_READ_INFO_BAD_PARENTS = 1,         /* parents whose status is not 0 */
  HF3FS_CLIENT_READ_INFO_HARD_PARENTS = 2,        /* parents whose status is not in {0, 7007}: an error a
                                                     block record cannot express */
  HF3FS_CLIENT_READ_INFO_WORDS = 4                /* (word 3 is written as 0) */
};

/* What the client does with a completed batchRead, for n_ios IOs and n_parents parents, on the
 * device and without a host round trip between the two steps.
 *
 * Verify (StorageClientImpl.cc:1720-1737), with HF3FS_CLIENT_READ_VERIFY only: a child with
 * status_in == 0 and read_len > 0 (:1722) is hashed in the type the server answered with (:1723);
 * a NONE-typed child computes {NONE, 0} without reading a byte (Common.h:150), so it mismatches
 * exactly when the server's value is not 0.  A mismatch (:1726) makes the child's result
 * IOResult(7015) (:1733): status 7015, and for the merge its checksum is {NONE, 0}.  Bad records
 * get status 3 and are not hashed: a child with status_in == 0 whose type is unknown (> CRC32)
 * or, with VERIFY, neither NONE nor `type` (the rule of hf3fs_crc_read_result_batch), or, with
 * VERIFY, whose read_len exceeds max_len or its own `length`, or whose data is 0 with
 * read_len > 0.  Every child gets `computed` and `status`.  Without VERIFY no data byte is read
 * and `data` may be anything; both CRC types may then occur in one batch.
 *
 * Merge (:1607-1633): parent p owns children [d_parent_off[p], d_parent_off[p+1]) of d_ios
 * (offsets ascending, the last one n_ios; an offset past n_ios is clamped); a null d_parent_off
 * means every IO is its own parent and needs n_parents == n_ios.  The first child whose status
 * after the verify is not 0 takes over (:1621-1623): the parent gets its status and its checksum
 * fields (those of IOResult(7015) after a mismatch), length 0, and failed_child.  Otherwise child
 * 0 is assigned (:1625); each later child adds its read_len in uint32_t (:1629) and is combined
 * (:1630) by ChecksumInfo::combine (src/fbs/storage/Common.h:179-198) with the return value
 * dropped: a parent typed otherwise than the child stays as it is (:180-183, the length was
 * added already), read_len 0 changes nothing (:184), a NONE parent adopts the child's checksum
 * (:186-188), else the CRC combine (:190-196).  A parent without children keeps IOResult's
 * default: status 7003, {NONE, 0}.
 *
 * d_blocks[p], when given, is the record FileWrapper::readFile builds from the parent
 * (src/client/cli/admin/FileWrapper.cc:132-163) and hf3fs_crc_file_digest_batch_ex takes:
 * read_len = length, block_len, checksum, checksum_type, missing = (status == 7007).
 * d_info[HF3FS_CLIENT_READ_INFO_*] is set, not accumulated.  d_parents or d_blocks may be NULL,
 * both with VERIFY: the parents are merged all the same and d_info counts them in every mode.
 *
 * HF3FS_CRC_INVALID_ARG before a device is touched: a type other than CRC32C / CRC32, unknown
 * flag bits, null d_ios with n_ios > 0, null d_info, null d_parent_off with n_parents != n_ios,
 * d_parents and d_blocks both null without VERIFY, a count above 2^30.  n_ios == 0 with
 * n_parents == 0 only zeroes d_info.  max_children >= every parent's child count chooses the
 * schedule (one lane or one wave per parent); a parent with more children is still merged
 * correctly.  max_len >= every read_len that is hashed.
 *
 * Asynchronous on `stream`, no host synchronisation, nothing read back; capturable, also as the
 * process's first library call, and a replayed graph works from what the records hold at replay
 * time.  No store goes to a caller data buffer. */
int hf3fs_crc_client_read_batch(uint8_t type, hf3fs_crc_client_read_io *d_ios, uint64_t n_ios,
                                const uint64_t *d_parent_off, uint64_t n_parents, uint64_t max_children,
                                uint32_t max_len, uint32_t flags, hf3fs_crc_client_read_result *d_parents,
                                hf3fs_crc_block_digest *d_blocks, uint32_t *d_info, void *stream);
/* Bytes of library-owned scratch one call of this shape takes with VERIFY (without it: none);
 * 0 for rejected counts. */
size_t hf3fs_crc_client_read_scratch_bytes(uint64_t n_ios, uint64_t n_parents);

/* ------------------------------------------------------------------------ */
/* client batchWrite: the checks and checksums before the send, the fold after */
/* ------------------------------------------------------------------------ */
/* One WriteIO of StorageClientImpl::batchWrite (src/client/storage/StorageClientImpl.cc:889-951,
 * 994-1015, 1878-1901 read the request fields; FileWrapper::writeFile,
 * src/client/cli/admin/FileWrapper.cc:218-248, reads the answer). */
typedef struct hf3fs_crc_client_write_io {
  uint64_t data;              /* device address of writeIO->data */
  uint64_t buf_base;          /* writeIO->buffer->data(); 0: buffer == nullptr */
  uint64_t buf_size;          /* the IOBuffer's capacity */
  uint32_t offset, length, chunk_size;
  /* outputs of prepare */
  uint32_t checksum;          /* writeIO->checksum.value (raw) */
  uint8_t  checksum_type;
  uint8_t  send_inline;       /* 1: length <= max_inline_bytes */
  uint8_t  reserved0[2];
  int32_t  status;            /* 0: to be sent; 7002; 3 for a bad record */
  /* the answer: inputs of complete (written by complete only with FROM_UPDATES) */
  int32_t  status_in;         /* 0, or result.lengthInfo.error().code(); 7003 when never sent */
  uint32_t result_len;        /* *result.lengthInfo */
  uint32_t result_checksum;   /* result.checksum.value (raw) */
  uint8_t  result_checksum_type;
  uint8_t  reserved1[3];
} hf3fs_crc_client_write_io;  /* 64 bytes */

/* What writeFile returns for one file: the fold of its IOs' answers. */
typedef struct hf3fs_crc_client_write_file {
  uint64_t length;            /* sum of the folded succLength; 0 when status != 0 */
  uint32_t value;             /* the folded checksum value (raw); 0 when status != 0 */
  uint8_t  type;              /* the folded checksum type; NONE when status != 0 */
  uint8_t  reserved[3];
  int32_t  status;            /* 0, or the code that ended the fold */
  uint32_t failed_io;         /* index in d_ios of the IO that ended the fold, ~0u if none */
} hf3fs_crc_client_write_file; /* 24 bytes */

enum { HF3FS_CRC_CLIENT_INVALID_ARG = 7002 };     /* StorageClientCode::kInvalidArg (:223) */
enum { HF3FS_CLIENT_WRITE_VERIFY = 1,             /* prepare: options.verifyChecksum() (:1880) */
       HF3FS_CLIENT_WRITE_FROM_UPDATES = 2 };     /* complete: the answers are d_updates' outputs */
enum {                                            /* words of hf3fs_crc_client_write_prepare's d_info */
  HF3FS_CLIENT_WRITE_INFO_SENT = 0,               /* IOs with status 0 */
  HF3FS_CLIENT_WRITE_INFO_RANGE = 1,              /* IOs that failed their own range check (7002, rule 2) */
  HF3FS_CLIENT_WRITE_INFO_BAD_RECORDS = 2,        /* IOs with length > max_len (3, rule 1) */
  HF3FS_CLIENT_WRITE_INFO_POISONED = 3,           /* 0 / 1: the buffer check failed the batch (rule 3) */
  HF3FS_CLIENT_WRITE_INFO_INLINE = 4,             /* sent IOs with send_inline */
  HF3FS_CLIENT_WRITE_INFO_HASHED_LO = 5,          /* bytes hashed: the lengths of the individually valid IOs */
  HF3FS_CLIENT_WRITE_INFO_HASHED_HI = 6,          /*   with VERIFY (also those of a poisoned batch), 64 bits */
  HF3FS_CLIENT_WRITE_INFO_WORDS = 8               /* (word 7 is written as 0) */
};
enum {                                            /* words of hf3fs_crc_client_write_complete's d_info */
  HF3FS_CLIENT_WRITE_DONE_FAILED = 0,             /* IOs whose final status is not 0 (collectFailedOps, :211-236) */
  HF3FS_CLIENT_WRITE_DONE_OK = 1,                 /* numProcessedChunks: IOs whose final status is 0 */
  HF3FS_CLIENT_WRITE_DONE_LEN_LO = 2,             /* totalDataLen (:1958-1968): result_len over the OK IOs, */
  HF3FS_CLIENT_WRITE_DONE_LEN_HI = 3,             /*   64 bits */
  HF3FS_CLIENT_WRITE_DONE_BAD_FILES = 4,          /* files whose status is not 0 */
  HF3FS_CLIENT_WRITE_DONE_MISMATCHED_FILES = 5,   /* files with 7015 (d_expected) */
  HF3FS_CLIENT_WRITE_DONE_WORDS = 8               /* (words 6 and 7 are written as 0) */
};

/* What batchWrite does with n WriteIOs before it sends them, on the device.  Per IO, in this order:
 *
 * 1. A bad record: length > max_len gives status 3.  The IO is not hashed, is not sent and takes no
 *    part in rule 3.
 * 2. Its own range (validateWriteDataRange, :994-1015): chunk_size == 0 or
 *    (uint32_t)(offset + length) > chunk_size gives 7002 for this IO alone; the sum is the
 *    reference's uint32_t arithmetic and wraps.  The IO takes no part in rule 3.
 * 3. The buffer check (validateDataRange, :889-951) over the IOs that passed 1 and 2: if one of them
 *    has buf_base == 0, data == 0 or is not contained in its buffer (RDMABuf.h:162: buf_base <= data
 *    and data + length <= buf_base + buf_size, in 64-bit unsigned sums; a sum that wraps counts as not
 *    contained), every one of them gets 7002 and nothing is sent: the batch is poisoned.  The
 *    overlap check behind check_overlapping_write_buffers (default false) stays with the host.
 * 4. The checksum of a sent IO (sendWriteRequest, :1878-1896): with HF3FS_CLIENT_WRITE_VERIFY
 *    {type, raw CRC of data[0, length)}, for length 0 {type, ~0u} with no byte read; without it
 *    {NONE, 0} and no data byte is read.  send_inline = (length <= max_inline_bytes) (:1898-1901).
 *    An IO that is not sent gets {NONE, 0} and send_inline 0.
 *
 * Reads: only the payload of an IO that is valid by itself (it passes 1 and 2, data and buf_base are
 * not 0, it is contained) is ever read, and only with VERIFY; it may be read although another IO
 * poisons the batch.  No other address is read, and no store goes to a data buffer.
 *
 * d_updates, when not NULL, receives the request as the server's record: for a sent IO payload =
 * data, offset, length, update_type = HF3FS_UPDATE_WRITE, write_checksum_type, write_checksum and
 * flags = 0; for an IO that is not sent update_type = 0 only (hf3fs_crc_update_batch answers 3 and
 * touches nothing).  No other byte of the record is stored: the chunk's address and state are the
 * server's.  d_info[HF3FS_CLIENT_WRITE_INFO_*] is set, not accumulated. */
int hf3fs_crc_client_write_prepare(uint8_t type, hf3fs_crc_client_write_io *d_ios, uint64_t n, uint32_t max_len,
                                   uint32_t max_inline_bytes, uint32_t flags, hf3fs_crc_update_io *d_updates,
                                   uint32_t *d_info, void *stream);

/* What the client and writeFile do with the answers.  With HF3FS_CLIENT_WRITE_FROM_UPDATES an IO
 * with status == 0 first takes its answer from d_updates[i] (status_in = status, result_len =
 * length, result_checksum(_type) = out_checksum(_type)) and the four fields are stored into d_ios.
 * An IO's final status is status != 0 ? status : status_in (setResultOfOp, :1922; an IO never sent
 * arrives with 7003).
 *
 * Fold (FileWrapper.cc:218-248): file f owns IOs [d_file_off[f], d_file_off[f+1]) (ascending,
 * clamped to n); NULL d_file_off with n_files == 0 skips it.  In file order: a final status != 0
 * ends the fold with that code; result_checksum_type > CRC32 ends it with 3; result_len != length
 * with 33; else ChecksumInfo::combine (Common.h:179-198): an accumulator typed otherwise than the
 * answer ends it with 4080 (also for result_len 0), result_len 0 changes nothing, a NONE
 * accumulator adopts the answer, else the CRC combine; result_len is added to `length`.  The
 * answer's checksum is the CHUNK's after the update, so the fold is the CRC of the written bytes
 * only when every IO starts its chunk.  A file whose fold ended gets length 0, {NONE, 0}, the code
 * and failed_io; a file without IOs {0, 0, NONE, status 0}.  d_expected[f], when given
 * (Bench.cc:41-48): a file with status 0 and value != d_expected[f] gets 7015, failed_io ~0u.
 * max_ios_per_file >= every file's IO count chooses the schedule (one lane or one wave per file);
 * the records are the same under either.
 *
 * d_failed, when given, is the ascending list of the IOs whose final status is not 0, written up
 * to failed_cap entries; d_info[HF3FS_CLIENT_WRITE_DONE_FAILED] is their full count.
 *
 * Both calls: HF3FS_CRC_INVALID_ARG before a device is touched for a type other than CRC32C /
 * CRC32, unknown flag bits, null d_ios with n > 0, null d_info, a count above 2^30,
 * FROM_UPDATES without d_updates, n_files > 0 with null d_file_off or null d_files, failed_cap > 0
 * with null d_failed.  n == 0 only sets d_info, and the file records when there are files.
 * Asynchronous on `stream`, no host synchronisation, nothing read back; capturable, also as the
 * process's first library calls, and a replayed graph works from what the records hold at replay
 * time. */
int hf3fs_crc_client_write_complete(hf3fs_crc_client_write_io *d_ios, uint64_t n, const uint64_t *d_file_off,
                                    uint64_t n_files, uint64_t max_ios_per_file, uint32_t flags,
                                    const hf3fs_crc_update_io *d_updates, const uint32_t *d_expected,
                                    hf3fs_crc_client_write_file *d_files, uint32_t *d_failed, uint64_t failed_cap,
                                    uint32_t *d_info, void *stream);
/* Bytes of library-owned scratch either call takes for n IOs (the larger of the two, so the pair's
 * buffer never grows between them); 0 for rejected counts. */
size_t hf3fs_crc_client_write_scratch_bytes(uint64_t n, uint64_t n_files);

/* ------------------------------------------------------------------------ */
/* chain forwarding: the hop between a target's local update and its commit   */
/* ------------------------------------------------------------------------ */
/* One update on a head or middle target between its local update and its commit:
 * StorageOperator::handleUpdate (src/storage/service/StorageOperator.cc:401-485) around
 * ReliableForwarding::forward / doForward (src/storage/service/ReliableForwarding.cc:113-134,
 * 145-278).  The host fills the inputs from the request, the local IOResult and the target,
 * hf3fs_crc_forward_prepare decides and builds the outgoing request, the host sends it and writes
 * the successor's answer into the response fields, hf3fs_crc_forward_complete decides the commit.
 * Checksums are raw, as everywhere at this ABI.  No call writes one of its own inputs. */
typedef struct hf3fs_crc_forward_job {
  /* request (UpdateReq.payload / .options / .featureFlags) */
  uint64_t payload;              /*   0 device address of rdmabuf (`length` bytes; 0 for truncate / extend / remove) */
  uint64_t chunk;                /*   8 device address of the chunk bytes [0, chunk_len): the syncing read */
  uint32_t offset;               /*  16 UpdateIO.offset */
  uint32_t length;               /*  20 UpdateIO.length */
  uint32_t chunk_size;           /*  24 UpdateIO.chunkSize */
  uint32_t req_update_ver;       /*  28 UpdateIO.updateVer as the request carries it (0: unset) */
  uint32_t req_checksum;         /*  32 UpdateIO.checksum.value */
  uint8_t update_type;           /*  36 HF3FS_UPDATE_{WRITE,REMOVE,TRUNCATE,EXTEND} */
  uint8_t req_checksum_type;     /*  37 UpdateIO.checksum.type */
  uint8_t req_flags;             /*  38 HF3FS_FORWARD_REQ_* */
  uint8_t upd_checksum_type;     /*  39 updateResult.checksum.type */
  /* local update result (doUpdate's IOResult) */
  int32_t upd_status;            /*  40 0, or lengthInfo.error().code() */
  uint32_t upd_length;           /*  44 *lengthInfo */
  uint32_t upd_update_ver;       /*  48 */
  uint32_t upd_commit_ver;       /*  52 */
  uint32_t upd_checksum;         /*  56 updateResult.checksum.value */
  /* target */
  uint32_t chain_ver;            /*  60 target->vChainId.chainVer */
  uint8_t has_successor;         /*  64 target->successor.has_value() */
  uint8_t successor_syncing;     /*  65 successor's publicState == SYNCING */
  uint8_t engine_job;            /*  66 chunkEngineJob.chunk() != nullptr */
  uint8_t chunk_checksum_type;   /*  67 state_.chunkChecksum.type */
  /* chunk: what the syncing read (ReliableForwarding.cc:160-190) or queryChunk (:216) finds */
  uint32_t chunk_len;            /*  68 state_.chunkLen */
  uint32_t chunk_checksum;       /*  72 state_.chunkChecksum.value */
  uint32_t chunk_update_ver;     /*  76 readResult.updateVer / chunkResult->updateVer */
  uint32_t chunk_commit_chain_ver; /* 80 batch.front().result().commitChainVer */
  int32_t chunk_status_in;       /*  84 0, or the code the read / queryChunk failed with */
  /* outputs of prepare */
  uint64_t out_data;             /*  88 updateReq.payload.rdmabuf: `payload`, or `chunk` after a syncing read */
  int32_t status;                /*  96 0 for a job that goes on; what a RETURN job answers */
  uint32_t res_length;           /* 100 updateResult after rung A (zeros after 4082 and a bad record) */
  uint32_t res_update_ver;       /* 104 */
  uint32_t res_commit_ver;       /* 108 */
  uint32_t out_offset;           /* 112 the outgoing request: zeros unless action == SEND */
  uint32_t out_length;           /* 116 */
  uint32_t out_checksum;         /* 120 */
  uint32_t out_update_ver;       /* 124 */
  uint32_t out_commit_chain_ver; /* 128 updateReq.options.commitChainVer, valid with HF3FS_FORWARD_OUT_COMMIT_CHAIN_VER */
  uint32_t computed;             /* 132 the chunk's re-hashed value where the syncing read computed one, else 0 */
  uint8_t action;                /* 136 HF3FS_FORWARD_{RETURN,SEND,NO_SUCCESSOR} */
  uint8_t is_syncing;            /* 137 commitIO.isSyncing (:152) */
  uint8_t out_update_type;       /* 138 */
  uint8_t out_checksum_type;     /* 139 */
  uint8_t out_flags;             /* 140 HF3FS_FORWARD_OUT_* */
  /* the successor's response: written by the host for SEND jobs, preset by prepare for the others */
  uint8_t fwd_checksum_type;     /* 141 */
  uint8_t reserved0[2];          /* 142 */
  int32_t fwd_status;            /* 144 0, or result.lengthInfo.error().code() (also a transport error's code) */
  uint32_t fwd_length;           /* 148 */
  uint32_t fwd_checksum;         /* 152 */
  uint32_t fwd_commit_ver;       /* 156 */
  uint32_t fwd_commit_chain_ver; /* 160 */
  /* outputs of complete (prepare presets commit_ver and commit_chain_ver, see below) */
  int32_t final_status;          /* 164 0 for COMMIT; what a RETURN job answers */
  uint32_t commit_ver;           /* 168 commitIO.commitVer */
  uint32_t commit_chain_ver;     /* 172 commitIO.commitChainVer */
  uint32_t fwd_update_ver;       /* 176 forwardResult.updateVer as :251 sets it (is_syncing and forward ok), else 0:
                                        the response's own updateVer stands */
  uint32_t buffer_computed;      /* 180 the outgoing buffer's re-hashed value where complete computed one, else 0 */
  uint8_t final_action;          /* 184 HF3FS_FORWARD_COMMIT or HF3FS_FORWARD_RETURN */
  uint8_t buffer_corrupted;      /* 185 1: the re-hash after a 4080 answer differs from out_checksum (:268) */
  uint8_t reserved1[6];          /* 186 */
} hf3fs_crc_forward_job;         /* 192 bytes */

enum { HF3FS_FORWARD_REQ_SYNCING = 1,  /* req.options.isSyncing */
       HF3FS_FORWARD_REQ_INLINE = 2 }; /* FeatureFlags::SEND_DATA_INLINE set in req.featureFlags */
enum { HF3FS_FORWARD_OUT_SYNCING = 1,  /* updateReq.options.isSyncing */
       HF3FS_FORWARD_OUT_INLINE = 2,   /* SEND_DATA_INLINE in updateReq.featureFlags */
       HF3FS_FORWARD_OUT_COMMIT_CHAIN_VER = 4 }; /* doForward set options.commitChainVer (:155,201); clear: the
                                                    request's own value goes out */
enum { HF3FS_FORWARD_RETURN = 1,       /* handleUpdate co_returns: `status` / `final_status` and the res_ fields */
       HF3FS_FORWARD_SEND = 2,         /* messenger.update(out_...) to the successor, then complete */
       HF3FS_FORWARD_NO_SUCCESSOR = 3, /* :113-117: nothing to send, complete commits */
       HF3FS_FORWARD_COMMIT = 4 };     /* doCommit with commit_ver / commit_chain_ver / is_syncing */
enum {                                 /* words of hf3fs_crc_forward_prepare's d_info */
  HF3FS_FORWARD_INFO_SENT = 0,
  HF3FS_FORWARD_INFO_RETURNED = 1,
  HF3FS_FORWARD_INFO_NO_SUCCESSOR = 2,
  HF3FS_FORWARD_INFO_SYNC_HASHED = 3,     /* syncing reads whose chunk bytes were hashed */
  HF3FS_FORWARD_INFO_SYNC_MISMATCHED = 4, /* syncing reads answered 4080 (NONE-typed ones included) */
  HF3FS_FORWARD_INFO_BAD_RECORDS = 5,     /* status 3 */
  HF3FS_FORWARD_INFO_WORDS = 8            /* both calls; words without a name are written as 0 */
};
enum {                                 /* words of hf3fs_crc_forward_complete's d_info */
  HF3FS_FORWARD_DONE_COMMITS = 0,      /* entries of d_commit_idx */
  HF3FS_FORWARD_DONE_RETURNED = 1,     /* final_action RETURN, prepare's RETURN jobs included */
  HF3FS_FORWARD_DONE_7015 = 2,
  HF3FS_FORWARD_DONE_4081 = 3,
  HF3FS_FORWARD_DONE_4082 = 4,         /* rung D's only; prepare's are `status` already */
  HF3FS_FORWARD_DONE_REHASHED = 5,     /* outgoing buffers hashed after a 4080 answer */
  HF3FS_FORWARD_DONE_CORRUPTED = 6,    /* buffer_corrupted set */
  HF3FS_FORWARD_DONE_UNHASHABLE = 7    /* 4080 answers whose buffer cannot be hashed (see below): not compared */
};

/* hf3fs_crc_forward_prepare, per job, in this order.
 *
 * A record whose update_type is none of WRITE / REMOVE / TRUNCATE / EXTEND is RETURN 3.
 *
 * A. The local result (StorageOperator.cc:401-434).  upd_status 0: a req_update_ver of 0 becomes
 * upd_update_ver (:404-405; "the request's version" below is that value, the input field is not
 * written), any other that differs is RETURN 4082 (:406-409).  4007 and 4012: RETURN the local
 * result as it is (:411-414, 427-430).  4008: RETURN status 0 with res_length = length and
 * res_update_ver = res_commit_ver = the request's version (:415-421).  4006: go on with
 * res_length = length, res_update_ver = the request's version (:422-426).  Any other code: RETURN
 * it (:431-434).  A job that goes on has commit_ver = res_update_ver (:441).
 *
 * B. forward / doForward (ReliableForwarding.cc:113-222).  No successor: action NO_SUCCESSOR,
 * commit_chain_ver = chain_ver (:115), the response fields preset to fwd_status 4033 and zeros.
 * Otherwise is_syncing = successor_syncing (:152), and the syncing read is taken when the type is
 * WRITE / TRUNCATE / EXTEND, is_syncing, and REQ_SYNCING or length != chunk_size (:158-159).
 *   With it: a non-zero chunk_status_in is RETURNed (:190).  A chunk type that is neither NONE nor
 *   `type`, chunk_len > max_len, or a null `chunk` with chunk_len > 0 is RETURN 3 and nothing is
 *   hashed.  Else the bytes [0, chunk_len) are hashed in chunk_checksum_type and compared with
 *   chunk_checksum (AioReadJob::setResult, src/storage/aio/BatchReadJob.cc:43-54): a NONE chunk
 *   computes {NONE, 0} without a byte read and mismatches exactly when chunk_checksum != 0; a
 *   mismatch is RETURN 4080.  On success the outgoing request is a WRITE of [0, chunk_len) from
 *   `chunk` with the stored chunk checksum, out_update_ver = chunk_update_ver, SYNCING set, INLINE
 *   set iff chunk_len <= max_inline_bytes (:193-212), out_commit_chain_ver =
 *   chunk_commit_chain_ver with REQ_SYNCING, else chain_ver (:155,200-202).  The checksum
 *   setResult leaves in result_ at BatchReadJob.cc:28-35 is never read by doForward: it is not
 *   computed here.  aioFinishRead's version check (:38) stays with the host: its failure is a
 *   chunk_status_in.
 *   Without it: the outgoing request is the request with the request's version; with is_syncing,
 *   not REMOVE and not engine_job a non-zero chunk_status_in is RETURNed and out_update_ver =
 *   chunk_update_ver (:215-222); with is_syncing SYNCING is set and out_commit_chain_ver =
 *   chain_ver (:153-156).
 * RETURN jobs get zeroed out_ and response fields and commit_ver = commit_chain_ver = 0.
 *
 * hf3fs_crc_forward_complete, per job.  A job whose action is not SEND or NO_SUCCESSOR keeps its
 * status: final_action RETURN, final_status = status.  For the others:
 *
 * C. The response (ReliableForwarding.cc:233-278, 120-134).  fwd_status 0: chain_ver <
 * fwd_commit_chain_ver turns the forward result into 4081 (:238-245); otherwise commit_ver =
 * fwd_commit_ver, commit_chain_ver = fwd_commit_chain_ver (:121-123) and, with is_syncing,
 * fwd_update_ver = the request's version (:251).  forward's own check (:125) is restated after
 * it and can never fire: doForward answered 4081 for the same condition already.  fwd_status
 * 4080: the outgoing buffer [out_data, out_length) is hashed in out_checksum_type and compared
 * with out_checksum (:263-268); a difference sets buffer_corrupted, and raising the signal
 * (:269-274) is the host's.  A NONE type computes {NONE, 0}; a type that is neither NONE nor
 * `type`, out_length > max_len or a null out_data with out_length > 0 is counted UNHASHABLE and not
 * compared.  The forward result stays 4080.
 *
 * D. handleUpdate after the forward (StorageOperator.cc:446-485).  commit_ver != res_update_ver:
 * RETURN 4082 (:446-453).  Forward ok: a REMOVE with fwd_checksum_type or upd_checksum_type NONE,
 * or with is_syncing, passes (:465-474); otherwise {type, value} inequality of fwd_checksum and
 * upd_checksum is RETURN 7015 (:475-482).  A forward error other than 4033 is RETURNed as it is
 * (:483-485).  Everything else is COMMIT with final_status 0.  Complete reads no field it writes,
 * so a job the host resent (forwardWithRetry's loop and its waiting are the host's) is completed
 * again by another call.
 *
 * d_commit_idx (n words, may be NULL) receives the COMMIT jobs' indices in ascending order, their
 * count goes to d_info[HF3FS_FORWARD_DONE_COMMITS].
 *
 * Both calls: asynchronous on `stream`, nothing synchronised or read back; capturable, also as a
 * process's first library call, and a replayed graph works from what the records hold at replay
 * time.  d_info (HF3FS_FORWARD_INFO_WORDS words) is set, not accumulated.  max_len >= every length
 * that is hashed.  HF3FS_CRC_INVALID_ARG before a device is touched: a type other than CRC32C /
 * CRC32, null d_jobs with n > 0, null d_info, n above 2^30.  n == 0 only zeroes d_info.  Only the
 * existing range kernels load data bytes, and only of the jobs that hash; no store goes to a
 * caller data buffer. */
int hf3fs_crc_forward_prepare(uint8_t type, hf3fs_crc_forward_job *d_jobs, uint64_t n, uint32_t max_len,
                              uint32_t max_inline_bytes, uint32_t *d_info, void *stream);
int hf3fs_crc_forward_complete(uint8_t type, hf3fs_crc_forward_job *d_jobs, uint64_t n, uint32_t max_len,
                               uint32_t *d_commit_idx, uint32_t *d_info, void *stream);
/* An upper bound of the library-owned scratch either call takes for n jobs on any device.  Both
 * calls take the same bytes for n jobs, whatever max_len is (prepare takes complete's share and
 * both reserve the tables of the byte-run schedule large prepares hash with), so the pair rule of
 * hf3fs_crc_update_scratch_bytes holds in n alone: after one call of either kind at the largest n
 * nothing grows.  Monotone in n, 0 for n above 2^30. */
size_t hf3fs_crc_forward_scratch_bytes(uint64_t n);

/* ------------------------------------------------------------------------ */
/* the storage server's batchRead (StorageOperator::batchRead)  */
/* ------------------------------------------------------------------------ */
/* One record per ReadIO of every reaped BatchReadReq, one record per request; request r owns jobs
 * [d_req_off[r], d_req_off[r+1]) of d_jobs (d_req_off: n_reqs + 1 non-decreasing offsets,
 * d_req_off[0] == 0, d_req_off[n_reqs] == n; an offset above n is read as n, so no record outside
 * the arrays is touched whatever the offsets hold).  Every decision is plain C++ in
 * 3fs_amd/csrc/server_read_plan.h. */
typedef struct hf3fs_crc_server_read_job {
  /* in: ReadIO */
  uint64_t remote_addr;    /* rdmabuf.addr() */
  uint64_t inner_offset;   /* in, chunk at prepare: meta.innerOffset / fd_and_offset().offset */
  /* in, completion (the host fills them when it builds the iocbs and reaps the events) */
  uint64_t localbuf;       /* device address of the aligned read: [localbuf, +read_len) */
  int64_t res;             /* io_event.res */
  /* out */
  uint64_t read_offset;    /* prepare: inner_offset + (offset - head_len) */
  uint64_t inline_off;     /* complete: byte offset in d_inline (0 for a job that packs nothing) */
  /* in: ReadIO */
  uint32_t offset, length, rdmabuf_size, rkey;
  /* in: target, chunk at prepare */
  int32_t target_status;   /* 0, or the code of getByChainId's error */
  int32_t meta_status;     /* 0, or the lookup's code (4001, 4002) */
  uint32_t commit_ver;     /* in; an engine job's is overwritten by update_ver in prepare */
  uint32_t update_ver, chain_ver, chunk_len, chunk_checksum;
  /* in, completion */
  int32_t meta_status_now; /* aioFinishRead's lookup */
  uint32_t update_ver_now;
  /* out of prepare */
  uint32_t head_len, tail_len, read_len, buf_ordinal, buf_off;
  int32_t status;
  /* out of complete */
  uint32_t result_len;
  int32_t result_status;
  uint32_t checksum;
  /* in */
  uint8_t has_rkey, up_to_date, engine, chunk_checksum_type;
  /* out */
  uint8_t buf_kind;        /* prepare: HF3FS_SERVER_READ_BUF_* */
  uint8_t checksum_type;   /* complete */
  uint8_t reserved[50];
} hf3fs_crc_server_read_job;   /* 192 bytes */

typedef struct hf3fs_crc_server_read_req {
  /* out of prepare */
  uint64_t total_len, total_head, total_tail;
  /* out of complete */
  uint64_t inline_off, inline_bytes, wr_bytes;
  /* in */
  uint32_t max_msg_sz;     /* port_.attr().max_msg_sz of the request's socket */
  /* out of prepare */
  int32_t status;
  uint32_t failed_job;     /* index in d_jobs; HF3FS_SERVER_READ_NONE without a failure */
  uint32_t n_small, n_big;
  /* out of complete */
  uint32_t n_ok, wr_first, wr_count, wr_fails;
  /* in */
  uint8_t checksum_type;   /* BatchReadReq::checksumType */
  uint8_t xmit;            /* HF3FS_SERVER_READ_XMIT_* */
  uint8_t read_uncommitted, recalculate;
  uint8_t reserved[40];
} hf3fs_crc_server_read_req;   /* 128 bytes */

typedef struct hf3fs_crc_server_read_wr {
  uint64_t remote_addr, local_addr;
  uint32_t length, rkey, job, req;
} hf3fs_crc_server_read_wr;    /* 32 bytes */

enum {
  HF3FS_SERVER_READ_XMIT_RDMA = 0,    /* neither flag: addBufferToBatch */
  HF3FS_SERVER_READ_XMIT_INLINE = 1,  /* FeatureFlags::SEND_DATA_INLINE: copyToRespBuffer */
  HF3FS_SERVER_READ_XMIT_NONE = 2     /* FeatureFlags::BYPASS_RDMAXMIT */
};
enum { HF3FS_SERVER_READ_BUF_NONE = 0, HF3FS_SERVER_READ_BUF_SMALL = 1, HF3FS_SERVER_READ_BUF_BIG = 2 };
#define HF3FS_SERVER_READ_NONE 0xFFFFFFFFu
enum {
  /* hf3fs_crc_server_read_prepare */
  HF3FS_SERVER_READ_INFO_REQS_OK = 0,
  HF3FS_SERVER_READ_INFO_REQS_FAILED = 1,
  HF3FS_SERVER_READ_INFO_JOBS_OK = 2,      /* jobs with status 0 */
  HF3FS_SERVER_READ_INFO_JOBS_FAILED = 3,
  HF3FS_SERVER_READ_INFO_SMALL = 4,        /* buffers over the passing requests */
  HF3FS_SERVER_READ_INFO_BIG = 5,
  /* hf3fs_crc_server_read_complete */
  HF3FS_SERVER_READ_DONE_OK = 0,           /* jobs with result_status 0 */
  HF3FS_SERVER_READ_DONE_FAILED = 1,
  HF3FS_SERVER_READ_DONE_INLINE_LO = 2,    /* bytes the inline arena needs, 64 bits */
  HF3FS_SERVER_READ_DONE_INLINE_HI = 3,
  HF3FS_SERVER_READ_DONE_INLINE_OVERFLOW = 4, /* 1: they exceed inline_cap, no inline byte was stored */
  HF3FS_SERVER_READ_DONE_WR = 5,           /* RDMA writes listed (the full count, beyond wr_cap too) */
  HF3FS_SERVER_READ_DONE_WR_FAILS = 6,
  HF3FS_SERVER_READ_DONE_HASHED = 7,       /* jobs whose bytes were hashed */
  HF3FS_SERVER_READ_INFO_WORDS = 8         /* both calls; words without a name are written as 0 */
};

/* The server's half of batchRead around the AIO, as two stream-ordered calls (DESIGN.md 3.11,
 * INTEGRATION.md 2.7).  Reference lines are of src/storage/.
 *
 * hf3fs_crc_server_read_prepare covers service/StorageOperator.cc:98-155, aio/BatchReadJob.cc:16-22,
 * store/ChunkReplica.cc:38-76 and store/ChunkEngine.h:34-73, per request in job order:
 *
 * 1. Alignment (BatchReadJob.cc:20-21), in the reference's wrapping uint32_t arithmetic:
 *    head_len = offset % 4096, tail_len = (4096 - (offset + length) % 4096) % 4096, read_len =
 *    length + head_len + tail_len (always a multiple of 4096).
 * 2. The first loop (StorageOperator.cc:101-130).  The first job that fails ends the request;
 *    within a job: target_status != 0 gives that code (:107-111), !up_to_date 4032 (:113-117),
 *    length > rdmabuf_size 3 (:122-128).  total_len / total_head / total_tail cover the jobs of a
 *    request that passes this loop, and are 0 for one that does not.
 * 3. The carve (StorageOperator.cc:141-154 over BufferPool::Buffer::tryAllocate / allocate,
 *    service/BufferPool.cc:102-141), only after the first loop has passed every job: a next-fit
 *    walk.  With no current buffer, or fewer than read_len bytes left in it, a new one is taken:
 *    read_len > big_buf fails the request with 2019 (the reference answers kRDMANoBuf for every
 *    allocation failure, :147-151), read_len > small_buf takes a big buffer, anything else a small
 *    one.  The job takes read_len bytes from the current buffer, big or small; later jobs go on
 *    taking from it.  buf_ordinal counts the request's buffers from 0 in the order taken, buf_kind
 *    is the buffer's kind and buf_off the offset in it; n_small and n_big count the request's
 *    buffers (0 for a failed request).  alignBuffer (:17-25) never moves: every read_len is a
 *    multiple of 4096.
 * 4. A failed request: status is the code, failed_job the failing job's index in d_jobs; every job
 *    of it has that status, read_len 0 and no buffer.
 * 5. Every job of a passing request, aioPrepareRead: meta_status != 0 is this job's status alone
 *    (ChunkReplica.cc:46-50, ChunkEngine.h:48-54).  An engine job stores commit_ver := update_ver
 *    in place (:61-62); its stored checksum reads as {CRC32C, ~chunk_checksum} (:65) in complete
 *    and nothing is checked.  A replica job with commit_ver != update_ver and no read_uncommitted
 *    gets 4004 (ChunkReplica.cc:61-66).  read_offset = inner_offset + (offset - head_len) (:72).
 * Prepare loads and stores records only.  One lane walks one request: the walk is sequential by
 * nature.  max_jobs_per_req (an upper bound of a request's jobs, 0 when unknown) has no effect at
 * present: it is accepted so that a later schedule for long requests needs no new signature, and a
 * request of many jobs is one lane's work.
 *
 * hf3fs_crc_server_read_complete covers aio/AioStatus.cc:27-55, aio/BatchReadJob.cc:24-113,
 * store/ChunkReplica.cc:79-100, store/StorageTarget.cc:299-304 and common/net/ib/IBSocket.cc:258-275.
 * A job whose prepare status is not 0 takes part in no rung: result_status is that status,
 * result_len 0, the checksum {NONE, 0}.  A record this call cannot serve gets result_status 3 the
 * same way: a request checksum_type or a stored checksum type that is neither NONE nor `type`, a
 * clipped length above max_len, or a null localbuf under bytes that are hashed or packed.  The
 * other jobs:
 *
 * 1. The length clip (AioStatus.cc:27-55): res < 0 gives 4010 with {NONE, 0}; otherwise L =
 *    min(max(0, res - head_len), length, max(0, chunk_len - offset)) in signed 64 bits.
 * 2. Rung 1 of setResult (BatchReadJob.cc:26-35) with the request's checksum_type T: NONE gives
 *    {NONE, 0}; T equal to the stored type with offset == 0 and L == chunk_len gives the stored
 *    checksum; anything else the raw CRC of [localbuf + head_len, +L), {T, ~0u} for L == 0 with
 *    no byte read.
 * 3. aioFinishRead (:38, StorageTarget.cc:299-304), replica jobs only: meta_status_now != 0 gives
 *    that code, update_ver != update_ver_now 4004 (ChunkReplica.cc:85-98).
 * 4. The recalculation (:43-54).  The reference dereferences lengthInfo here even when rung 3 has
 *    just made it an error; this call skips the rung then.  With recalculate, offset == 0 and L ==
 *    chunk_len the bytes are hashed with the stored type and a value other than the stored one
 *    gives 4080; a NONE stored type mismatches exactly when its stored value is not 0.  The
 *    same hashed range serves rungs 2 and 4.
 *    On every error result_len is 0 and the checksum fields keep rung 2's value.
 * 5. Inline (requests with xmit 1, BatchReadJob.cc:96-113): the L bytes of the jobs with
 *    result_status 0 are concatenated in job order into d_inline, the requests back to back in
 *    request order -- per request the layout StorageClientImpl.cc:1697-1717 consumes.  The job's
 *    and the request's inline_off are set (a request's is where its first byte would go),
 *    d_info holds the bytes needed.  When they exceed inline_cap no inline byte is stored at all
 *    and HF3FS_SERVER_READ_DONE_INLINE_OVERFLOW is 1; every other output is set all the same.
 * 6. The RDMA list (requests with xmit 0, BatchReadJob.cc:74-94): the jobs with result_status 0 in
 *    job order; one with localbuf == 0, !has_rkey, L > rdmabuf_size or L > max_msg_sz
 *    (IBSocket.cc:261-262) gets result_status 3 instead and counts in wr_fails.  A job of length
 *    0 is listed: its buffer is valid.  d_wr receives the list up to wr_cap entries,
 *    d_info[HF3FS_SERVER_READ_DONE_WR] its full length; a request's writes are wr_first,
 *    wr_count of the full list.
 * n_ok counts a request's jobs with result_status 0.
 *
 * Only the existing range kernels load bytes of [localbuf + head_len, +L) to hash, and only of
 * the jobs that hash.  The inline pack is the library's one kernel that stores payload bytes to a
 * caller buffer: a launch of its own behind the hash, the copy body of the update apply.
 *
 * The host keeps: BYPASS_DISKIO requests, the chunk lookup itself (it hands in meta_status and the
 * metadata), the buffer semaphore and the turning of buf_ordinal into addresses, the AIO, the RDMA
 * post and its failure fan-out (StorageOperator.cc:219-223), fault injection.
 *
 * Both calls: asynchronous on `stream`, nothing synchronised or read back; capturable, also as a
 * process's first library calls, and a replayed graph works from what the records hold at replay
 * time.  d_info (HF3FS_SERVER_READ_INFO_WORDS words) is set, not accumulated.
 * HF3FS_CRC_INVALID_ARG before a device is touched: a type other than CRC32C / CRC32 (complete),
 * null d_jobs with n > 0, null d_reqs or null d_req_off with n_reqs > 0, n > 0 with n_reqs == 0,
 * null d_info, n or n_reqs above 2^30, inline_cap > 0 with null d_inline, wr_cap > 0 with null
 * d_wr. */
int hf3fs_crc_server_read_prepare(hf3fs_crc_server_read_job *d_jobs, uint64_t n,
                                  hf3fs_crc_server_read_req *d_reqs, const uint64_t *d_req_off, uint64_t n_reqs,
                                  uint64_t max_jobs_per_req, uint32_t small_buf, uint32_t big_buf,
                                  uint32_t *d_info, void *stream);
int hf3fs_crc_server_read_complete(uint8_t type, hf3fs_crc_server_read_job *d_jobs, uint64_t n,
                                   hf3fs_crc_server_read_req *d_reqs, const uint64_t *d_req_off, uint64_t n_reqs,
                                   uint32_t max_len, void *d_inline, uint64_t inline_cap,
                                   hf3fs_crc_server_read_wr *d_wr, uint64_t wr_cap, uint32_t *d_info, void *stream);
/* An upper bound of the library-owned scratch complete takes for n jobs of n_reqs requests on any
 * device (prepare takes none).  Monotone in n, 0 for counts above 2^30. */
size_t hf3fs_crc_server_read_scratch_bytes(uint64_t n, uint64_t n_reqs);

/* ------------------------------------------------------------------------ */
/* file MD5: admin `checksum --md5`                                           */
/* ------------------------------------------------------------------------ */
/* One run of bytes of a file, in file order. data == 0: `length` zero bytes (a hole). */
typedef struct hf3fs_crc_md5_seg {
  uint64_t data;            /* device address of the bytes (any alignment), 0 = a hole */
  uint64_t length;          /* bytes, 0 allowed */
} hf3fs_crc_md5_seg;

/* MD5_CTX between calls. tail[0, total % 64) = bytes not yet compressed; the call writes
 * the rest of tail as zero (and reserved as 0), so a state is a deterministic function of the
 * bytes seen. */
typedef struct hf3fs_crc_md5_state {
  uint32_t h[4];            /* A, B, C, D */
  uint64_t total;           /* message bytes seen so far, mod 2^64 (see below) */
  uint8_t tail[64];
  uint64_t reserved;
} hf3fs_crc_md5_state;

enum { HF3FS_MD5_INIT = 1, HF3FS_MD5_FINAL = 2 };

/* The MD5 leg of the admin command (src/client/cli/admin/Checksum.cc:50-83: MD5_Init, one
 * MD5_Update per buffer fill in file order through FileWrapper.cc:172-177, MD5_Final) for n_files
 * files at once, one GPU lane per file.  File f owns segments [d_file_off[f], d_file_off[f+1]) of
 * d_segs, the indexing of hf3fs_crc_file_digest_batch; its message is the concatenation of its
 * segments' bytes.  Segments may have any address alignment and any length, 0 included; a file
 * may have no segments.  n_segs is the caller's statement of d_file_off[n_files] (the call reads
 * nothing back); a wrong n_segs is undefined behaviour.
 * HF3FS_MD5_INIT: every file starts from the RFC 1321 initial state; without it file f continues
 * from d_state[f].  HF3FS_MD5_FINAL: the padding and the 64-bit bit length (total * 8 mod 2^64)
 * are applied and d_out[16 f .. 16 f + 16) receives the digest in MD5_Final's byte order;
 * d_state[f], when given, is left unchanged (the state before the padding).  Without FINAL
 * d_state[f] receives the running state and d_out is ignored.  d_state == NULL needs INIT | FINAL
 * (the one-shot form); a call with neither flag is a pure MD5_Update.  One call per buffer fill
 * with d_state carried is the reference's loop.
 * total is a full 64-bit count and wraps at 2^64 bytes.  The wrap loses nothing the digest needs:
 * total % 64 and total * 8 mod 2^64 are the same before and after it, and the bit count mod 2^64 is
 * all MD5_Update keeps (Nl, Nh), so a stream that passes 2^64 bytes still gets MD5_Final's digest.
 * Holes -- a deliberate difference: data == 0 hashes zeros.  The reference's `--md5 --fillZero`
 * hashes whatever its unzeroed RDMA buffer held for a hole (FileWrapper.cc:140-152 never touches
 * the buffer), a quirk and no contract; this call gives the MD5 of the file with holes as zeros,
 * which is what the CRC leg computes for the same option.
 * Errors, all checked before any device is touched: n_files == 0 is OK; null d_file_off, n_segs >
 * 0 with null d_segs, unknown flag bits, d_state == NULL unless both flags are set, FINAL with
 * null d_out, n_files or n_segs above 2^30 -> kInvalidArg.
 * Aliasing: d_out and d_state overlap no segment and not each other; anything else is undefined.
 * Stream behaviour follows hf3fs_crc_sync_plan: asynchronous on `stream`, no host synchronisation,
 * nothing read back; capturable, also as the process's first library call; a replayed graph
 * re-plans from what d_segs, d_file_off and d_state hold at replay time.  Scratch per (stream,
 * thread) pair outside a capture and graph-owned inside one, never the stream-ordered pool; every
 * scratch word read is written by the call first (option poison).
 * Options honoured: md5_sort (1: lanes take the files bucketed by length, so the 64 files of a
 * wave end together; 0: in file order) and md5_stage (0: every lane loads its own 64 bytes; 1: the
 * wave stages the lanes' next pieces through LDS with coalesced loads).  The result is the same
 * under all four settings. */
int hf3fs_crc_md5_batch(const hf3fs_crc_md5_seg *d_segs, const uint64_t *d_file_off, uint64_t n_files,
                        uint64_t n_segs, hf3fs_crc_md5_state *d_state, uint8_t *d_out, uint32_t flags,
                        void *stream);
/* Bytes of scratch one such call takes, its full need: what a (stream, thread) pair's buffer
 * is sized to by a first call of n_files (12 bytes per file and a table of up to 256 KiB, rounded up to the
 * buffer's 256 KiB granule; a captured call's own memory is the unrounded figure).  Monotone in
 * n_files: after one call of the largest n_files nothing grows.  0 for a count the call rejects. */
size_t hf3fs_crc_md5_scratch_bytes(uint64_t n_files);
/* host: fmt "{:02x}" join of 16 digest bytes (Checksum.cc:148) into out32, no terminator; returns 32 */
uint32_t hf3fs_crc_md5_hex(const uint8_t *digest16, char *out32);

/* ------------------------------------------------------------------------ */
/* stored-chunk scrub against persisted checksums         */
/* ------------------------------------------------------------------------ */
/* One stored chunk and the checksum its metadata persists: either C++
 * ChunkMetadata {size, checksumType, checksumValue} (src/fbs/storage/
 * Common.h:652-677, raw value) or the chunk engine's ChunkMeta {len, checksum}
 * (src/storage/chunk_engine/src/types/chunk_meta.rs:7-20, finalized value,
 * type CRC32C, bridged with ~ at src/storage/store/ChunkEngine.cc:42,66). */
typedef struct hf3fs_crc_scrub_io {
  uint64_t data;            /* device address of the chunk bytes */
  uint32_t length;          /* ChunkMetadata.size / ChunkMeta.len */
  uint8_t checksum_type;    /* ChunkMetadata.checksumType (engine records: CRC32C) */
  uint8_t fin;              /* 1: `checksum` is finalized (ChunkMeta.checksum), 0: raw */
  uint16_t reserved;
  uint32_t checksum;        /* persisted value */
  uint32_t computed;        /* out: raw create(type, data, length) (0 for NONE) */
  int32_t status;           /* out: 0; 4080 on mismatch; 3 for a bad record */
  uint32_t reserved2;
} hf3fs_crc_scrub_io;

/* Recompute every typed chunk and compare with its persisted checksum, as the
 * full-chunk resync check of AioReadJob::setResult does per read
 * (BatchReadJob.cc:43-54).  NONE chunks pass unchecked.  Non-NONE types must
 * equal `type`.  *d_mismatch_count is SET to the number of non-zero statuses. */
int hf3fs_crc_scrub_batch(uint8_t type, hf3fs_crc_scrub_io *d_ios, uint64_t n, uint32_t max_len,
                          uint32_t *d_mismatch_count, void *stream);

/* ------------------------------------------------------------------------ */
/* resync plan: the comparison loop of ResyncWorker::handleSync               */
/* ------------------------------------------------------------------------ */
/* One chunk's metadata as the resync comparison reads it (src/storage/sync/ResyncWorker.cc:199-303):
 * a record of the local table is a ChunkMetadata of getAllMetadataMap, a record of the remote table
 * a ChunkMeta the successor returned from syncStart.  One layout serves both.  Chunk ids are the 16
 * bytes of ChunkId(high, low) (Common.cc:10-18); ids of any other length are outside this call. */
typedef struct hf3fs_crc_sync_meta {
  uint64_t id_hi, id_lo;    /* ChunkId(high, low) (Common.cc:10-18); equality only */
  uint32_t chain_ver;       /* ChunkMeta.chainVer / ChunkMetadata.chainVer */
  uint32_t update_ver, commit_ver;
  uint32_t checksum;        /* raw value */
  uint32_t length;          /* ChunkMeta.length / ChunkMetadata.size (carried, not compared) */
  uint32_t chunk_size;      /* local: innerFileId.chunkSize (the write list's second member); remote: 0 */
  uint8_t chunk_state;      /* ChunkState: COMMIT 0, DIRTY 1, CLEAN 2 */
  uint8_t recycle_state;    /* local: RecycleState, 0 = NORMAL; remote: 0 */
  uint8_t checksum_type;
  uint8_t out_class;        /* out: HF3FS_SYNC_* below */
  uint32_t out_peer;        /* out: index of the matched record in the other table, 0xFFFFFFFF if none */
} hf3fs_crc_sync_meta;

/* out_class of a remote record: the first rung of the ladder (ResyncWorker.cc:203-275) that holds;
 * "local" is the local record with the same id, chain_ver the call's argument. */
enum {
  HF3FS_SYNC_REMOTE_ONLY = 1,             /* no local record, or an earlier remote record with this id took
                                             it (:205-210): remove at the successor */
  HF3FS_SYNC_LOCAL_RECYCLING = 2,         /* local.recycle_state != NORMAL (:215-219): nothing */
  HF3FS_SYNC_CHAIN_VER_LOW = 3,           /* local.chain_ver > remote.chain_ver: forward */
  HF3FS_SYNC_REMOTE_UNCOMMITTED = 4,      /* remote update_ver != commit_ver or state != COMMIT: forward */
  HF3FS_SYNC_REMOTE_CHAIN_VER_HIGH = 5,   /* local.chain_ver < remote's, local COMMIT: fatal */
  HF3FS_SYNC_LOCAL_UNCOMMITTED = 6,       /* the same, local not COMMIT: skip */
  HF3FS_SYNC_COMMIT_VER_MISMATCH = 7,     /* local.update_ver != remote.commit_ver, local.chain_ver !=
                                             chain_ver, local COMMIT: fatal */
  HF3FS_SYNC_CHAIN_WRITING = 8,           /* local.update_ver != remote.commit_ver otherwise: skip */
  HF3FS_SYNC_FULL_SYNC_HEAVY = 9,         /* flag HF3FS_SYNC_HEAVY: forward */
  HF3FS_SYNC_CHECKSUM_MISMATCH = 10,      /* {type, value} differ (Common.h:200), local.chain_ver !=
                                             chain_ver: fatal */
  HF3FS_SYNC_CHAIN_WRITING_CHECKSUM = 11, /* {type, value} differ otherwise: skip */
  HF3FS_SYNC_EQUAL = 12,                  /* skip */
  /* out_class of a local record */
  HF3FS_SYNC_MATCHED = 16,     /* a remote record took it: out_peer = the lowest-indexed remote record
                                  with its id (also when the record is recycling) */
  HF3FS_SYNC_REMOTE_MISS = 17, /* no remote record has its id: forward (:289-292), recycling or not */
  HF3FS_SYNC_DUPLICATE = 18    /* an earlier local record has the same id (the reference's table is a
                                  map: it cannot happen there).  Never matched, never forwarded */
};

/* Words of d_info. */
enum {
  HF3FS_SYNC_INFO_FATAL = 0,               /* 0 or 1 (hasFatalEvents) */
  HF3FS_SYNC_INFO_FIRST_FATAL = 1,         /* lowest remote index with a fatal class, else 0xFFFFFFFF */
  HF3FS_SYNC_INFO_N_WRITE = 2,
  HF3FS_SYNC_INFO_N_REMOVE = 3,
  HF3FS_SYNC_INFO_RECYCLE = 4,             /* storage.syncing.chunk_in_recycle_state */
  HF3FS_SYNC_INFO_CHAIN_VER_LOW = 5,       /* .chain_version_low */
  HF3FS_SYNC_INFO_REMOTE_UNCOMMITTED = 6,  /* .remote_uncommitted */
  HF3FS_SYNC_INFO_CHAIN_VER_HIGH = 7,      /* .chain_version_high */
  HF3FS_SYNC_INFO_LOCAL_UNCOMMITTED = 8,   /* .local_uncommitted */
  HF3FS_SYNC_INFO_COMMIT_VER_MISMATCH = 9, /* .commit_version_mismatch */
  HF3FS_SYNC_INFO_CHAIN_WRITING = 10,      /* .current_chain_is_writing (both of its rungs) */
  HF3FS_SYNC_INFO_FULL_SYNC_HEAVY = 11,    /* .full_sync_heavy */
  HF3FS_SYNC_INFO_FULL_SYNC_LIGHT = 12,    /* .full_sync_light */
  HF3FS_SYNC_INFO_SKIP = 13,               /* .skip_count: LOCAL_UNCOMMITTED, both CHAIN_WRITING classes and
                                              EQUAL; not LOCAL_RECYCLING (:218 continues before :273), not a
                                              fatal record */
  HF3FS_SYNC_INFO_REMOTE_MISS = 14,        /* .remote_miss_count */
  HF3FS_SYNC_INFO_DUPLICATES = 15,         /* local records of class DUPLICATE (whole table, fatal or not) */
  HF3FS_SYNC_INFO_WORDS = 16
};
enum { HF3FS_SYNC_HEAVY = 1 }; /* flags: FullSyncLevel::HEAVY for this chain (:102-105) */

/* The comparison loop as one stream-ordered call: a hash join of the two tables on the 128-bit id,
 * then the ladder.  Writes out_class and out_peer of every record of both tables (a record's class
 * does not depend on the break below) and all HF3FS_SYNC_INFO_WORDS words of d_info.
 * Break: the reference stops at the first fatal record (:232,243,256) and builds no lists
 * (:277-287).  So with fatal == 1 the ladder counters (words 4-13) cover the remote records
 * [0, first_fatal] -- what the reference's local variables hold at the break -- remote_miss, n_write
 * and n_remove are 0 and the list contents are unspecified.
 * Lists (fatal == 0): d_write (capacity n_local) receives, ascending, the local indices to forward:
 * MATCHED records whose peer is CHAIN_VER_LOW, REMOTE_UNCOMMITTED or FULL_SYNC_HEAVY, and
 * REMOTE_MISS records.  d_remove (capacity n_remote) receives, ascending, the REMOTE_ONLY remote
 * indices.  The reference's own order is remote order followed by unordered_map order, which is
 * unspecified, and the forwards are independent of each other: ascending index is this call's.
 * Either list pointer may be NULL; the counts are set all the same.
 * Errors, all checked before any device is touched: null d_info, a null table with a non-zero
 * count, unknown flag bits, n_local or n_remote above 2^30 -> kInvalidArg.  n_local == n_remote
 * == 0 is OK: d_info is the empty plan.
 * Stream behaviour follows hf3fs_crc_update_ordered: asynchronous on `stream`, no host
 * synchronisation, nothing read back; capturable, also as the process's first library call; a
 * replayed graph re-plans from what the tables hold at replay time.  Scratch per (stream, thread)
 * pair outside a capture and graph-owned inside one, never the stream-ordered pool; every scratch
 * word read is written by the call first (option poison). */
int hf3fs_crc_sync_plan(hf3fs_crc_sync_meta *d_local, uint64_t n_local, hf3fs_crc_sync_meta *d_remote,
                        uint64_t n_remote, uint32_t chain_ver, uint32_t flags, uint32_t *d_write,
                        uint32_t *d_remove, uint32_t *d_info, void *stream);
/* Bytes of scratch one such call takes: after one call of the largest (n_local, n_remote) nothing
 * grows.  0 for counts the call rejects. */
size_t hf3fs_crc_sync_plan_scratch_bytes(uint64_t n_local, uint64_t n_remote);

/* Plan -> recheck without a host round trip: turns the plan's write list into n_local scrub
 * records.  d_addrs[i] is the device address of local chunk i; n_write is read from d_info on the
 * device.  Record k < n_write describes local record d_write[k]: data, length, checksum_type, raw
 * checksum, fin 0.  Every other record is {data 0, length 0, type NONE}, which
 * hf3fs_crc_scrub_batch passes unchecked: the caller runs hf3fs_crc_scrub_batch(type, d_scrub,
 * n_local, ...) on the same stream.  Null arguments with n_local > 0 -> kInvalidArg; n_local == 0
 * is OK. */
int hf3fs_crc_sync_scrub_fill(const hf3fs_crc_sync_meta *d_local, const uint64_t *d_addrs, const uint32_t *d_write,
                              const uint32_t *d_info, uint64_t n_local, hf3fs_crc_scrub_io *d_scrub, void *stream);

/* ------------------------------------------------------------------------ */
/* chunk range walks: queryLastChunk, removeChunks and the file-length fold  */
/* ------------------------------------------------------------------------ */
/* One QueryLastChunkOp or RemoveChunksOp payload: a walk over one target's chunk metadata by
 * chunk-id range (StorageOperator::queryLastChunk, src/storage/service/StorageOperator.cc:858-916,
 * and ::removeChunks, :936-1000, both through processQueryResults, :653-751, over
 * ChunkStore::queryChunks, src/storage/store/ChunkStore.cc:120-147).  Ids compare as the unsigned
 * pair (hi, lo): the byte order of ChunkId(high, low) (Common.cc:10-18). */
typedef struct hf3fs_crc_range_op {
  uint64_t begin_hi, begin_lo; /* ChunkIdRange [begin, end) */
  uint64_t end_hi, end_lo;
  uint32_t max_chunks;         /* maxNumChunkIdsToProcess; 0 = unlimited */
  int32_t status_in;           /* a failure the host found before the walk (getByChainId, :638); non-zero:
                                  status = status_in and nothing is walked */
  uint8_t kind;                /* HF3FS_RANGE_QUERY or HF3FS_RANGE_REMOVE; anything else: status 3 */
  uint8_t reserved0[3];
  uint32_t chain_id;           /* carried; hf3fs_crc_file_length reads it */
  uint64_t last_hi, last_lo;   /* out: lastChunkId, the highest processed id; 0, 0 when none */
  uint64_t total_len;          /* out: totalChunkLen, the sum of the processed records' length */
  uint32_t total_chunks;       /* out: totalNumChunks / the upper bound of numChunksRemoved */
  uint32_t last_len;           /* out: lastChunkLen */
  uint32_t last_index;         /* out: table index of the last chunk, 0xFFFFFFFF when none */
  uint32_t list_first;         /* out: where the op's segment of d_list begins (0xFFFFFFFF: past 32 bits) */
  int32_t status;              /* out: 0, status_in, or 3 (bad kind, unsorted table) */
  uint8_t more;                /* out: moreChunksInRange */
  uint8_t reserved1[3];
} hf3fs_crc_range_op;

enum { HF3FS_RANGE_QUERY = 1, HF3FS_RANGE_REMOVE = 2 };

/* Words of hf3fs_crc_range_query's d_info. */
enum {
  HF3FS_RANGE_INFO_OPS_OK = 0,     /* ops with status 0 */
  HF3FS_RANGE_INFO_OPS_FAILED = 1, /* ops with status != 0 */
  HF3FS_RANGE_INFO_CHUNKS_LO = 2,  /* the sum of total_chunks, 64 bits */
  HF3FS_RANGE_INFO_CHUNKS_HI = 3,
  HF3FS_RANGE_INFO_LIST_LO = 4,    /* list entries of all REMOVE ops, 64 bits (also past list_cap) */
  HF3FS_RANGE_INFO_LIST_HI = 5,
  HF3FS_RANGE_INFO_OVERFLOW = 6,   /* 1 when the list entries exceed list_cap */
  HF3FS_RANGE_INFO_UNSORTED = 7,   /* indices i >= 1 with id[i-1] >= id[i] */
  HF3FS_RANGE_INFO_WORDS = 8
};

/* n_ops range walks over one target's table d_meta[0, n_meta) (the layout hf3fs_crc_sync_plan takes,
 * read only here), as one stream-ordered call.  The table must be strictly ascending by (id_hi,
 * id_lo); the call counts the indices that break the order in d_info[UNSORTED], and when there is
 * one every op gets status 3, no outputs and an empty list segment.
 * Per op, the closed form of the paged loop (:653-751):
 *   span          the records with begin <= id < end (none when begin >= end)
 *   normals       the span's records with recycle_state == 0 (:677-696 skips the others)
 *   limit         max_chunks ? min(max_chunks, 2^32 - 2) : 2^32 - 2 (:658-660)
 *   total_chunks  min(normals, limit);  more = normals > limit
 *   processed     the total_chunks normal records of the span with the highest ids (the walk
 *                 descends from `end`); last_* describe the highest, total_len sums their length
 * The page size max_num_results_per_query changes no output.  An op that is not walked (status !=
 * 0) has last_index 0xFFFFFFFF and every other output 0 but list_first and status.
 * The list: a REMOVE op's processed records' table indices go to d_list[list_first, list_first +
 * total_chunks), highest id first: the order in which removeChunks issues doRemove (:949-971).
 * Segments lie in op order, list_first is the sum of the earlier ops' list counts (a QUERY op lists
 * nothing and carries the running offset), entries at positions >= list_cap are not written (d_info
 * has the full count and the overflow flag).  Ranges of different ops may overlap.
 * Errors, all checked before any device is touched: null d_info, a null array with a non-zero
 * count, n_meta or n_ops above 2^30, null d_list with list_cap > 0 -> kInvalidArg.  Both counts 0 is
 * OK: d_info is the empty result.
 * Stream behaviour follows hf3fs_crc_sync_plan: asynchronous on `stream`, no host synchronisation,
 * nothing read back; capturable, also as the process's first library call; a replayed graph
 * re-plans from what table and ops hold at replay time.  Scratch per (stream, thread) pair outside
 * a capture and graph-owned inside one; every scratch word read is written by the call first. */
int hf3fs_crc_range_query(const hf3fs_crc_sync_meta *d_meta, uint64_t n_meta, hf3fs_crc_range_op *d_ops,
                          uint64_t n_ops, uint32_t *d_list, uint64_t list_cap, uint32_t *d_info, void *stream);
/* Bytes of scratch one such call takes; 0 for counts the call rejects. */
size_t hf3fs_crc_range_query_scratch_bytes(uint64_t n_meta, uint64_t n_ops);

/* One file of the meta service's length query (FileOperation::queryChunksByChain / queryChunks,
 * src/fbs/meta/FileOperation.cc:45-179): its ops are d_ops[first_op, first_op + n_file_ops), the
 * file's stripes in order; n_file_ops is the reference's maxStripe. */
typedef struct hf3fs_crc_file_len {
  uint64_t inode;
  uint32_t first_op, n_file_ops;
  uint32_t chunk_size, stripe_size; /* layout.chunkSize, layout.stripeSize */
  uint8_t flags;                    /* HF3FS_FILE_LEN_DYN: dynStripe && inode.dynStripe */
  uint8_t reserved[3];
  int32_t status;                   /* out: 0, an op's status, 2, 3019, or 3 (a bad record) */
  uint64_t length;                  /* out: the greatest chunk * chunk_size + last_len over the chains */
  uint64_t total_len;               /* out: totalChunkLen, summed over the chains */
  uint64_t total_chunks;            /* out: totalNumChunks, summed over the chains */
  uint32_t last_chunk;              /* out: the winning chain's lastChunk */
  uint32_t last_chunk_len;          /* out: its lastChunkLen */
} hf3fs_crc_file_len;

enum { HF3FS_FILE_LEN_DYN = 1 };
enum { HF3FS_FILE_LEN_MAX_OPS = 1024 };

/* Words of hf3fs_crc_file_length's d_info. */
enum {
  HF3FS_FILE_LEN_INFO_OK = 0,        /* files with status 0 */
  HF3FS_FILE_LEN_INFO_FAILED = 1,    /* files with status != 0 */
  HF3FS_FILE_LEN_INFO_EMPTY = 2,     /* files with status 0 and no surviving op */
  HF3FS_FILE_LEN_INFO_NOT_FOUND = 3, /* ops skipped for status 7007 (those before a file's first failing op) */
  HF3FS_FILE_LEN_INFO_BUSY = 4,      /* files with status 3019 */
  HF3FS_FILE_LEN_INFO_CORRUPT = 5,   /* files with status 2 */
  HF3FS_FILE_LEN_INFO_WORDS = 8      /* words 6 and 7 are 0 */
};

/* The fold of n_files files over finished range ops (d_ops is read only).  Per file, over its ops in
 * order (:127-176): status 7007 (kChunkNotFound) skips the op; any other non-zero status ends the
 * file with that code; total_chunks == 0 skips the op; last id == meta::ChunkId(InodeId(-1), 0, 0)
 * or inode(id) != inode ends the file with 2 (kDataCorruption), where inode(id) = ((last_hi &
 * 0xFFFFFFFFFFFF) << 16) | (last_lo >> 48) and chunk(id) = last_lo & 0xFFFFFFFF (the big-endian
 * layout of src/fbs/meta/Schema.h:177-226); with DYN set, n_file_ops < stripe_size and chunk(id) >=
 * n_file_ops the file ends with 3019 (MetaCode::kBusy).  Otherwise the op enters the map under its
 * chain_id with length = chunk(id) * chunk_size + last_len (64 bits), replacing an earlier op of
 * the file with that chain_id.  The fold (:45-76), in ascending chain_id: the greatest length wins,
 * on equal lengths the lowest chain_id; total_len and total_chunks sum the map's entries.  A file
 * with no entry is all zeros with status 0; a file that ends with a code has that status and zero
 * outputs.  The kFoundBug check (:70) cannot fire with this arithmetic.
 * Bad records get status 3 and read no op: first_op + n_file_ops > n_ops, n_file_ops > 1024.
 * Segments of different files may overlap.
 * Errors before any device is touched: null d_info, a null array with a non-zero count, n_ops or
 * n_files above 2^30 -> kInvalidArg.  Stream, capture and poison contract as above; no scratch. */
int hf3fs_crc_file_length(const hf3fs_crc_range_op *d_ops, uint64_t n_ops, hf3fs_crc_file_len *d_files,
                          uint64_t n_files, uint32_t *d_info, void *stream);

/* The chunk engine's persisted ChunkMeta (chunk_meta.rs:7-20) in its derse
 * wire form: a one-byte body length, then pos u64, chain_ver, chunk_ver, len,
 * checksum (u32 each), timestamp, last_request_id, last_client_low/high (u64
 * each, all little-endian), etag (length byte + bytes), uncommitted (bool).
 * Pinned by the reference's own vector (chunk_meta.rs:59-87).  Bodies of 128
 * bytes or more use a multi-byte length whose derse encoding is not pinned by
 * any reference vector: rejected with kInvalidArg. */
typedef struct hf3fs_crc_engine_meta {
  uint64_t pos;
  uint32_t chain_ver;
  uint32_t chunk_ver;
  uint32_t len;
  uint32_t checksum;        /* finalized CRC32C of the chunk's [0, len) */
  uint64_t timestamp;
  uint64_t last_request_id;
  uint64_t last_client_low;
  uint64_t last_client_high;
  uint8_t etag_len;
  uint8_t uncommitted;
  uint8_t etag[62];
} hf3fs_crc_engine_meta;

int hf3fs_crc_engine_meta_decode(const void *h_bytes, uint64_t n, hf3fs_crc_engine_meta *out, uint64_t *consumed);
int hf3fs_crc_engine_meta_encode(const hf3fs_crc_engine_meta *m, void *h_out, uint64_t cap, uint64_t *written);
/* ChunkMeta::set_default_etag_if_need (chunk_meta.rs:30-34): format!("{:X}",
 * checksum) into out (no terminator); returns its length (1..8). */
uint32_t hf3fs_crc_default_etag(uint32_t checksum_fin, char *out8);

/* ------------------------------------------------------------------------ */
/* serde message frames                                   */
/* ------------------------------------------------------------------------ */
/* One framed message: MessageHeader {u32 checksum; u32 size} + payload
 * (src/common/net/MessageHeader.h:20-27). */
typedef struct hf3fs_crc_frame {
  uint64_t offset;          /* payload offset in the receive buffer (header at offset - 8) */
  uint32_t size;            /* MessageHeader.size */
  uint32_t checksum;        /* MessageHeader.checksum as received */
  uint32_t computed;        /* out: Checksum::calcSerde(payload, size, checksum & 1) */
  int32_t status;           /* out: 0; 4080 when computed != checksum; 3 for size > max_size */
} hf3fs_crc_frame;

/* The framing walk of Processor::unpackMsg (src/common/net/Processor.h:85-107)
 * over host bytes: records every complete serde frame in order (at most
 * max_frames).  Returns 0 when the buffer is a whole number of serde frames,
 * kInvalidArg at the first incomplete or non-serde frame (what the reference
 * treats as a broken transport); n_frames and consumed cover the frames before it. */
int hf3fs_crc_frame_walk(const void *h_buf, uint64_t len, hf3fs_crc_frame *h_frames, uint64_t max_frames,
                         uint64_t *n_frames, uint64_t *consumed);
/* Checksum::calcSerde (MessageHeader.h:33-37: crc32c with init 0, low byte =
 * 0x86 | compressed) of every frame payload at d_buf + offset, compared with
 * the received header (Processor.h:111-120).  `computed` also serves the send
 * side (WriteItem.h:100).  *d_mismatch_count is SET to the non-zero statuses. */
int hf3fs_crc_frame_verify_batch(const void *d_buf, hf3fs_crc_frame *d_frames, uint64_t n, uint32_t max_size,
                                 uint32_t *d_mismatch_count, void *stream);

/* ------------------------------------------------------------------------ */
/* host-memory entry points (synchronous)                                    */
/* ------------------------------------------------------------------------ */
/* ChecksumInfo::create over host buffers: bytes are streamed H2D through a
 * pinned staging ring (two streams) and hashed on the current device. */
int hf3fs_crc_create_host(uint8_t type, const void *const *h_bufs, const uint64_t *h_lens, const uint32_t *h_starts,
                          uint32_t *h_out, uint64_t n);

/* ------------------------------------------------------------------------ */
/* per-IO request coalescer                               */
/* ------------------------------------------------------------------------ */
/* The reference hashes one IO per call on the thread that completes it:
 * AioReadJob::setResult (src/storage/aio/BatchReadJob.cc:24-35, 32
 * AioReadWorker threads), ChunkReplica::update's payload verify
 * (src/storage/store/ChunkReplica.cc:193-207, 32 UpdateWorker threads) and the
 * client's per-IO create/verify (src/client/storage/StorageClientImpl.cc:
 * 1720-1737, 1878-1882).  A coalescer accepts such single ChecksumInfo::create
 * requests from any number of threads and hashes whatever arrived while the
 * previous batch was on the device in one launch. */
typedef struct hf3fs_crc_coalescer hf3fs_crc_coalescer;

/* Completion callback: status 0 and the raw value of create(type, buf, len,
 * start), or an error status and 0.  Runs on the coalescer's completion
 * thread, in launch order; it must not block. */
typedef void (*hf3fs_crc_done_fn)(void *arg, int status, uint32_t value);

typedef struct hf3fs_crc_coalescer_options {
  int device;            /* HIP device that hashes the requests */
  uint32_t max_batch;    /* requests per type per launch (default 4096) */
  uint32_t max_wait_us;  /* an idle device waits this long for company (default 0) */
  uint32_t slots;        /* batches open + in flight (default 4, >= 2) */
  uint32_t inflight;     /* launch early only while fewer batches are on the device (default 2, < slots) */
  uint32_t service_wgs;  /* 0: batch mode.  > 0: service mode, CRC32C requests are served by this many
                            resident workgroups polling a request ring (no launch per request) */
  uint64_t stage_bytes;  /* pinned stage per slot for HOST_COPY requests (default 32 MiB) */
  uint32_t service_ring;     /* service ring slots, power of two (default 1024) */
  uint32_t service_idle_us;  /* the service kernel exits after this long without requests and is
                                relaunched on demand (default 2000) */
  uint64_t service_stage;    /* pinned stage per ring slot for HOST_COPY requests (default 64 KiB;
                                larger requests take the batch path) */
} hf3fs_crc_coalescer_options;

/* request flags */
enum {
  /* `buf` is plain host memory: the submitting thread copies it into a pinned
   * stage that the kernel reads over PCIe.  Without the flag `buf` must be
   * device-accessible (HBM, or host memory from hf3fs_crc_host_register) and
   * stay valid until the callback runs. */
  HF3FS_CRC_REQ_HOST_COPY = 1
};

void hf3fs_crc_coalescer_default_options(hf3fs_crc_coalescer_options *opt); /* device = current device */
int hf3fs_crc_coalescer_create(const hf3fs_crc_coalescer_options *opt, hf3fs_crc_coalescer **out);
/* Launches what is pending, completes every request, joins the threads. */
void hf3fs_crc_coalescer_destroy(hf3fs_crc_coalescer *co);
/* Asynchronous ChecksumInfo::create(type, buf, len, start) (Common.h:146-177):
 * NONE -> value 0 and length 0 -> value `start` complete at once on the
 * calling thread.  A HOST_COPY request larger than stage_bytes is hashed
 * through hf3fs_crc_create_host before returning. */
int hf3fs_crc_coalescer_submit(hf3fs_crc_coalescer *co, uint8_t type, const void *buf, uint64_t len, uint32_t start,
                               uint32_t flags, hf3fs_crc_done_fn fn, void *arg);
/* Blocking form: returns the submit/batch status, *out = raw value. */
int hf3fs_crc_coalescer_create_one(hf3fs_crc_coalescer *co, uint8_t type, const void *buf, uint64_t len,
                                   uint32_t start, uint32_t flags, uint32_t *out);
/* out4 = {requests, batches launched, bytes, largest batch}.  requests: the accepted requests
 * that had bytes to hash (a type other than NONE and len > 0), whichever route took them (a
 * batch launch, the service ring, or hf3fs_crc_create_host for a HOST_COPY request larger than
 * stage_bytes); a request is counted when its submit call accepts it.  bytes: the sum of their
 * lengths.  batches launched: hf3fs_crc_create_batch launches (none for the other two routes).
 * largest batch: the most requests of one type in one launch, in the unit of options.max_batch
 * and never above it. */
int hf3fs_crc_coalescer_stats(hf3fs_crc_coalescer *co, uint64_t *out4);

/* Page-lock and map host memory (3FS registers its RDMA BufferPool slabs,
 * src/storage/service/BufferPool.h:24-27, and client IOBuffers the same way)
 * so kernels read it in place; *d_ptr is the device address of h_ptr. */
int hf3fs_crc_host_register(void *h_ptr, uint64_t len, void **d_ptr);
int hf3fs_crc_host_unregister(void *h_ptr);

/* Wait for `stream`'s queued work without spinning: hipStreamQuery polled with a sleep of
 * poll_us microseconds between polls (poll_us == 0: hipStreamSynchronize, HIP's busy wait).
 * For many caller threads on few cores -- 3FS's 32 AioReadWorker threads on a storage node's
 * CPU quota: 32 spinning waits on a 16-CPU quota were throttled by the cgroup for tens of
 * milliseconds at a time (p99 batch latency 58 ms against 4.3 ms polled). */
int hf3fs_crc_stream_wait(void *stream, uint32_t poll_us);

/* ------------------------------------------------------------------------ */
/* synthetic data (benchmarks/tests)                                         */
/* ------------------------------------------------------------------------ */
/* Fills n_chunks chunks of chunk_len bytes at d_dst + i*stride with
 * splitmix64(seed ^ ((first_chunk_id + i) << 32) ^ word_index) little-endian
 * words, byte-identical to oracle/orc_fill_synth. */
int hf3fs_crc_fill_synth(void *d_dst, uint64_t stride, uint64_t chunk_len, uint64_t n_chunks, uint64_t seed,
                         uint64_t first_chunk_id, void *stream);

#ifdef __cplusplus
}
/* hf3fs_crc_forward_job's layout is part of the ABI (3fs_amd/_lib.py mirrors it). */
static_assert(sizeof(hf3fs_crc_forward_job) == 192 && sizeof(hf3fs_crc_forward_job) % 8 == 0, "forward job size");
static_assert(offsetof(hf3fs_crc_forward_job, update_type) == 36 && offsetof(hf3fs_crc_forward_job, upd_status) == 40 &&
                  offsetof(hf3fs_crc_forward_job, chain_ver) == 60 && offsetof(hf3fs_crc_forward_job, chunk_len) == 68 &&
                  offsetof(hf3fs_crc_forward_job, chunk_status_in) == 84,
              "forward job inputs");
static_assert(offsetof(hf3fs_crc_forward_job, out_data) == 88 && offsetof(hf3fs_crc_forward_job, status) == 96 &&
                  offsetof(hf3fs_crc_forward_job, computed) == 132 && offsetof(hf3fs_crc_forward_job, action) == 136 &&
                  offsetof(hf3fs_crc_forward_job, out_flags) == 140,
              "forward job prepare outputs");
static_assert(offsetof(hf3fs_crc_forward_job, fwd_checksum_type) == 141 &&
                  offsetof(hf3fs_crc_forward_job, fwd_status) == 144 &&
                  offsetof(hf3fs_crc_forward_job, fwd_commit_chain_ver) == 160 &&
                  offsetof(hf3fs_crc_forward_job, final_status) == 164 &&
                  offsetof(hf3fs_crc_forward_job, final_action) == 184 &&
                  offsetof(hf3fs_crc_forward_job, buffer_corrupted) == 185,
              "forward job response and complete outputs");
/* The server read records' layouts are part of the ABI (3fs_amd/_lib.py mirrors them). */
static_assert(sizeof(hf3fs_crc_server_read_job) == 192 && sizeof(hf3fs_crc_server_read_job) % 64 == 0,
              "server read job size");
static_assert(offsetof(hf3fs_crc_server_read_job, localbuf) == 16 && offsetof(hf3fs_crc_server_read_job, res) == 24 &&
                  offsetof(hf3fs_crc_server_read_job, read_offset) == 32 &&
                  offsetof(hf3fs_crc_server_read_job, inline_off) == 40 &&
                  offsetof(hf3fs_crc_server_read_job, offset) == 48 &&
                  offsetof(hf3fs_crc_server_read_job, target_status) == 64 &&
                  offsetof(hf3fs_crc_server_read_job, meta_status_now) == 92 &&
                  offsetof(hf3fs_crc_server_read_job, head_len) == 100 &&
                  offsetof(hf3fs_crc_server_read_job, status) == 120 &&
                  offsetof(hf3fs_crc_server_read_job, result_len) == 124 &&
                  offsetof(hf3fs_crc_server_read_job, has_rkey) == 136 &&
                  offsetof(hf3fs_crc_server_read_job, buf_kind) == 140 &&
                  offsetof(hf3fs_crc_server_read_job, checksum_type) == 141,
              "server read job layout");
static_assert(sizeof(hf3fs_crc_server_read_req) == 128 && sizeof(hf3fs_crc_server_read_req) % 64 == 0,
              "server read request size");
static_assert(offsetof(hf3fs_crc_server_read_req, inline_off) == 24 && offsetof(hf3fs_crc_server_read_req, wr_bytes) == 40 &&
                  offsetof(hf3fs_crc_server_read_req, max_msg_sz) == 48 &&
                  offsetof(hf3fs_crc_server_read_req, status) == 52 &&
                  offsetof(hf3fs_crc_server_read_req, n_ok) == 68 &&
                  offsetof(hf3fs_crc_server_read_req, wr_fails) == 80 &&
                  offsetof(hf3fs_crc_server_read_req, checksum_type) == 84 &&
                  offsetof(hf3fs_crc_server_read_req, recalculate) == 87,
              "server read request layout");
static_assert(sizeof(hf3fs_crc_server_read_wr) == 32 && offsetof(hf3fs_crc_server_read_wr, length) == 16 &&
                  offsetof(hf3fs_crc_server_read_wr, req) == 28,
              "server read write-list entry layout");
/* The range records' layouts are part of the ABI (3fs_amd/_lib.py mirrors them). */
static_assert(sizeof(hf3fs_crc_range_op) == 96 && offsetof(hf3fs_crc_range_op, max_chunks) == 32 &&
                  offsetof(hf3fs_crc_range_op, status_in) == 36 && offsetof(hf3fs_crc_range_op, kind) == 40 &&
                  offsetof(hf3fs_crc_range_op, chain_id) == 44 && offsetof(hf3fs_crc_range_op, last_hi) == 48 &&
                  offsetof(hf3fs_crc_range_op, total_len) == 64 && offsetof(hf3fs_crc_range_op, total_chunks) == 72 &&
                  offsetof(hf3fs_crc_range_op, last_len) == 76 && offsetof(hf3fs_crc_range_op, last_index) == 80 &&
                  offsetof(hf3fs_crc_range_op, list_first) == 84 && offsetof(hf3fs_crc_range_op, status) == 88 &&
                  offsetof(hf3fs_crc_range_op, more) == 92,
              "range op layout");
static_assert(sizeof(hf3fs_crc_file_len) == 64 && offsetof(hf3fs_crc_file_len, first_op) == 8 &&
                  offsetof(hf3fs_crc_file_len, chunk_size) == 16 && offsetof(hf3fs_crc_file_len, flags) == 24 &&
                  offsetof(hf3fs_crc_file_len, status) == 28 && offsetof(hf3fs_crc_file_len, length) == 32 &&
                  offsetof(hf3fs_crc_file_len, total_chunks) == 48 && offsetof(hf3fs_crc_file_len, last_chunk) == 56 &&
                  offsetof(hf3fs_crc_file_len, last_chunk_len) == 60,
              "file length record layout");
#endif
#endif /* HF3FS_CRC_H */
