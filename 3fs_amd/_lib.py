"""ctypes binding of the C ABI in include/hf3fs_crc.h (libhf3fs_crc.so).

This is the Python-side view of the drop-in boundary used by tests, bench.py
and smoke().  It never computes a checksum itself: every call goes to the HIP
library, and a missing library raises instead of falling back to anything.
"""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
# HF3FS_CRC_LIB: load another build of the library (same-tree A/B of kernel variants)
LIB_PATH = os.environ.get("HF3FS_CRC_LIB") or os.path.join(HERE, "lib", "libhf3fs_crc.so")
HEADER = os.path.join(REPO, "include", "hf3fs_crc.h")

NONE, CRC32C, CRC32 = 0, 1, 2
UPDATE_WRITE, UPDATE_TRUNCATE, UPDATE_EXTEND = 1, 4, 8
MODE_REFERENCE, MODE_DELTA = 0, 1
OK, INVALID_ARG, CHUNK_READ_FAILED, CHECKSUM_MISMATCH, CLIENT_CHECKSUM_MISMATCH, DEVICE_ERROR = (
    0, 3, 4010, 4080, 7015, 9001)
SERDE_INSUFFICIENT_LENGTH = 40
NOT_APPLIED = 9002  # update_ordered: the IO was not reached (max_rounds); chunk untouched, resubmit it


class Hf3fsCrcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"hf3fs_crc error {code}: {msg}")
        self.code = code


class UpdateIO(ctypes.Structure):
    """hf3fs_crc_update_io (include/hf3fs_crc.h)."""
    _fields_ = [
        ("chunk", ctypes.c_uint64),
        ("payload", ctypes.c_uint64),
        ("offset", ctypes.c_uint32),
        ("length", ctypes.c_uint32),
        ("chunk_size", ctypes.c_uint32),
        ("update_type", ctypes.c_uint8),
        ("chunk_checksum_type", ctypes.c_uint8),
        ("write_checksum_type", ctypes.c_uint8),
        ("flags", ctypes.c_uint8),
        ("chunk_checksum", ctypes.c_uint32),
        ("write_checksum", ctypes.c_uint32),
        ("out_size", ctypes.c_uint32),
        ("out_checksum", ctypes.c_uint32),
        ("out_checksum_type", ctypes.c_uint8),
        ("checksum_case", ctypes.c_uint8),
        ("reserved1", ctypes.c_uint8 * 2),
        ("status", ctypes.c_int32),
    ]


assert ctypes.sizeof(UpdateIO) == 56
UPDATE_FLAG_ENGINE = 1
UPDATE_FLAG_SYNCING = 2  # a resync write: WRITE at offset 0, out_size = length, no old byte kept
FLAG_ENGINE, FLAG_SYNCING = UPDATE_FLAG_ENGINE, UPDATE_FLAG_SYNCING
DIGEST_FILL_ZERO = 1  # hf3fs_crc_file_digest_batch_ex flags
# UpdateIO.checksum_case (HF3FS_CKCASE_*): the reference's checksum counter for the IO
CKCASE_NONE, CKCASE_REUSE, CKCASE_COMBINE, CKCASE_RECOMPUTE = 1, 2, 3, 4


UPDATE_COMMIT = 16  # a commit job of update_versioned / update_engine (UpdateType::COMMIT)
CHUNK_STATE_COMMIT, CHUNK_STATE_DIRTY, CHUNK_STATE_CLEAN = 0, 1, 2
(CHUNK_NOT_CLEAN, CHUNK_STALE_UPDATE, CHUNK_MISSING_UPDATE, CHUNK_COMMITTED_UPDATE, CHUNK_ADVANCE_UPDATE,
 CHUNK_SIZE_MISMATCH, CHUNK_STALE_COMMIT, CHAIN_VERSION_MISMATCH, CHUNK_VERSION_MISMATCH) = (
    4005, 4006, 4007, 4008, 4012, 4015, 4023, 4081, 4082)
VER_INFO_WORDS = 8
VER_INFO_NAMES = ("chain_max", "not_applied", "updates", "commits", "refused", "fatal", "commit_dirty", "commit_stale")


def update_ver_dtype():
    """numpy dtype of hf3fs_crc_update_ver (include/hf3fs_crc.h): one 48-byte record per job."""
    import numpy as np
    return np.dtype([("io_ver", "<u4"), ("job_chain_ver", "<u4"), ("chain_ver", "<u4"), ("update_ver", "<u4"),
                     ("commit_ver", "<u4"), ("meta_chunk_size", "<u4"), ("chunk_state", "u1"), ("recycle_state", "u1"),
                     ("is_force", "u1"), ("reserved0", "u1"), ("out_chain_ver", "<u4"), ("out_update_ver", "<u4"),
                     ("out_commit_ver", "<u4"), ("out_chunk_state", "u1"), ("out_recycle_state", "u1"),
                     ("reserved1", "u1", (2,)), ("reserved2", "<u4")])


ENGINE_DETAIL_NONE, ENGINE_DETAIL_RECORD, ENGINE_DETAIL_IN_WRITING, ENGINE_DETAIL_NO_DST, ENGINE_DETAIL_NO_WRITING = range(5)
ENGINE_INFO_WORDS = 8
ENGINE_INFO_NAMES = ("chain_max", "not_applied", "updates", "commits", "refused", "cow", "in_place", "in_writing")


def engine_job_dtype():
    """numpy dtype of hf3fs_crc_engine_job (include/hf3fs_crc.h): one 104-byte record per job."""
    import numpy as np
    return np.dtype([("dst", "<u8"), ("addr", "<u8"), ("w_addr", "<u8"), ("out_addr", "<u8"), ("out_w_addr", "<u8"),
                     ("io_ver", "<u4"), ("job_chain_ver", "<u4"), ("chain_ver", "<u4"), ("chunk_ver", "<u4"),
                     ("w_len", "<u4"), ("w_checksum", "<u4"), ("w_chain_ver", "<u4"), ("w_chunk_ver", "<u4"),
                     ("out_chain_ver", "<u4"), ("out_chunk_ver", "<u4"), ("out_w_len", "<u4"),
                     ("out_w_checksum", "<u4"), ("out_w_chain_ver", "<u4"), ("out_w_chunk_ver", "<u4"),
                     ("out_cow", "u1"), ("detail", "u1"), ("reserved", "u1", (6,))])


class ReadIO(ctypes.Structure):
    """hf3fs_crc_read_io (include/hf3fs_crc.h): AioReadJob::setResult inputs/outputs."""
    _fields_ = [
        ("data", ctypes.c_uint64),
        ("offset", ctypes.c_uint32),
        ("length", ctypes.c_uint32),
        ("chunk_len", ctypes.c_uint32),
        ("batch_checksum_type", ctypes.c_uint8),
        ("chunk_checksum_type", ctypes.c_uint8),
        ("recalculate", ctypes.c_uint8),
        ("reserved0", ctypes.c_uint8),
        ("chunk_checksum", ctypes.c_uint32),
        ("out_checksum", ctypes.c_uint32),
        ("out_checksum_type", ctypes.c_uint8),
        ("reserved1", ctypes.c_uint8 * 3),
        ("status", ctypes.c_int32),
        ("reserved2", ctypes.c_uint32),
    ]


assert ctypes.sizeof(ReadIO) == 48


class BlockDigest(ctypes.Structure):
    """hf3fs_crc_block_digest: one chunk read of a file (FileWrapper.cc:133-160)."""
    _fields_ = [
        ("read_len", ctypes.c_uint64),
        ("block_len", ctypes.c_uint64),
        ("checksum", ctypes.c_uint32),
        ("checksum_type", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 3),
    ]


class FileDigest(ctypes.Structure):
    """hf3fs_crc_file_digest: ChecksumInfo of one file (or replica) + status."""
    _fields_ = [
        ("length", ctypes.c_uint64),
        ("value", ctypes.c_uint32),
        ("type", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 3),
        ("status", ctypes.c_int32),
        ("reserved2", ctypes.c_uint32),
    ]


assert ctypes.sizeof(BlockDigest) == 24 and ctypes.sizeof(FileDigest) == 24


class ClientReadIO(ctypes.Structure):
    """hf3fs_crc_client_read_io: one ReadIO of a completed batchRead (StorageClientImpl.cc:1720-1737)."""
    _fields_ = [
        ("data", ctypes.c_uint64),
        ("length", ctypes.c_uint32),
        ("read_len", ctypes.c_uint32),
        ("status_in", ctypes.c_int32),
        ("checksum", ctypes.c_uint32),
        ("checksum_type", ctypes.c_uint8),
        ("reserved0", ctypes.c_uint8 * 3),
        ("computed", ctypes.c_uint32),
        ("status", ctypes.c_int32),
        ("reserved1", ctypes.c_uint32),
    ]


class ClientReadResult(ctypes.Structure):
    """hf3fs_crc_client_read_result: parentIO->result after the merge (StorageClientImpl.cc:1607-1633)."""
    _fields_ = [
        ("length", ctypes.c_uint32),
        ("checksum", ctypes.c_uint32),
        ("checksum_type", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 3),
        ("status", ctypes.c_int32),
        ("failed_child", ctypes.c_uint32),
        ("block_len", ctypes.c_uint32),
    ]


assert ctypes.sizeof(ClientReadIO) == 40 and ctypes.sizeof(ClientReadResult) == 24
CLIENT_READ_VERIFY = 1  # hf3fs_crc_client_read_batch flags
CLIENT_NOT_INITIALIZED, CHUNK_NOT_FOUND = 7003, 7007
CLIENT_READ_INFO_WORDS = 4
CLIENT_READ_INFO_NAMES = ("bad_children", "bad_parents", "hard_parents", "reserved")
CLIENT_READ_NONE = 0xFFFFFFFF  # ClientReadResult.failed_child: no child took over


class ClientWriteIO(ctypes.Structure):
    """hf3fs_crc_client_write_io: one WriteIO of a batchWrite (StorageClientImpl.cc:889-951, 994-1015,
    1878-1901) and its answer (FileWrapper.cc:218-248)."""
    _fields_ = [
        ("data", ctypes.c_uint64),
        ("buf_base", ctypes.c_uint64),
        ("buf_size", ctypes.c_uint64),
        ("offset", ctypes.c_uint32),
        ("length", ctypes.c_uint32),
        ("chunk_size", ctypes.c_uint32),
        ("checksum", ctypes.c_uint32),
        ("checksum_type", ctypes.c_uint8),
        ("send_inline", ctypes.c_uint8),
        ("reserved0", ctypes.c_uint8 * 2),
        ("status", ctypes.c_int32),
        ("status_in", ctypes.c_int32),
        ("result_len", ctypes.c_uint32),
        ("result_checksum", ctypes.c_uint32),
        ("result_checksum_type", ctypes.c_uint8),
        ("reserved1", ctypes.c_uint8 * 3),
    ]


class ClientWriteFile(ctypes.Structure):
    """hf3fs_crc_client_write_file: what writeFile returns for one file."""
    _fields_ = [
        ("length", ctypes.c_uint64),
        ("value", ctypes.c_uint32),
        ("type", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 3),
        ("status", ctypes.c_int32),
        ("failed_io", ctypes.c_uint32),
    ]


assert ctypes.sizeof(ClientWriteIO) == 64 and ctypes.sizeof(ClientWriteFile) == 24
assert ClientWriteIO.status.offset == 44 and ClientWriteIO.result_checksum_type.offset == 60
CLIENT_INVALID_ARG, INVALID_FORMAT = 7002, 33
CLIENT_WRITE_VERIFY, CLIENT_WRITE_FROM_UPDATES = 1, 2  # flags of client_write_prepare / _complete
CLIENT_WRITE_INFO_WORDS = 8
CLIENT_WRITE_INFO_NAMES = ("sent", "range", "bad_records", "poisoned", "inline", "hashed_lo", "hashed_hi", "reserved")
CLIENT_WRITE_DONE_WORDS = 8
CLIENT_WRITE_DONE_NAMES = ("failed", "ok", "len_lo", "len_hi", "bad_files", "mismatched_files", "reserved0",
                           "reserved1")
CLIENT_WRITE_NONE = 0xFFFFFFFF  # ClientWriteFile.failed_io: no IO ended the fold


_u8c, _u32c, _i32c, _u64c = ctypes.c_uint8, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64


class ForwardJob(ctypes.Structure):
    """hf3fs_crc_forward_job: one update between its local update and its commit
    (StorageOperator.cc:401-485, ReliableForwarding.cc:113-278)."""
    _fields_ = [
        # request
        ("payload", _u64c), ("chunk", _u64c), ("offset", _u32c), ("length", _u32c), ("chunk_size", _u32c),
        ("req_update_ver", _u32c), ("req_checksum", _u32c), ("update_type", _u8c), ("req_checksum_type", _u8c),
        ("req_flags", _u8c), ("upd_checksum_type", _u8c),
        # local update result
        ("upd_status", _i32c), ("upd_length", _u32c), ("upd_update_ver", _u32c), ("upd_commit_ver", _u32c),
        ("upd_checksum", _u32c),
        # target
        ("chain_ver", _u32c), ("has_successor", _u8c), ("successor_syncing", _u8c), ("engine_job", _u8c),
        ("chunk_checksum_type", _u8c),
        # chunk
        ("chunk_len", _u32c), ("chunk_checksum", _u32c), ("chunk_update_ver", _u32c),
        ("chunk_commit_chain_ver", _u32c), ("chunk_status_in", _i32c),
        # outputs of prepare
        ("out_data", _u64c), ("status", _i32c), ("res_length", _u32c), ("res_update_ver", _u32c),
        ("res_commit_ver", _u32c), ("out_offset", _u32c), ("out_length", _u32c), ("out_checksum", _u32c),
        ("out_update_ver", _u32c), ("out_commit_chain_ver", _u32c), ("computed", _u32c), ("action", _u8c),
        ("is_syncing", _u8c), ("out_update_type", _u8c), ("out_checksum_type", _u8c), ("out_flags", _u8c),
        # the successor's response
        ("fwd_checksum_type", _u8c), ("reserved0", _u8c * 2), ("fwd_status", _i32c), ("fwd_length", _u32c),
        ("fwd_checksum", _u32c), ("fwd_commit_ver", _u32c), ("fwd_commit_chain_ver", _u32c),
        # outputs of complete
        ("final_status", _i32c), ("commit_ver", _u32c), ("commit_chain_ver", _u32c), ("fwd_update_ver", _u32c),
        ("buffer_computed", _u32c), ("final_action", _u8c), ("buffer_corrupted", _u8c), ("reserved1", _u8c * 6),
    ]


assert ctypes.sizeof(ForwardJob) == 192
UPDATE_REMOVE = 2  # hf3fs_crc_forward_job.update_type only
NO_SUCCESSOR_TARGET = 4033
FORWARD_REQ_SYNCING, FORWARD_REQ_INLINE = 1, 2
FORWARD_OUT_SYNCING, FORWARD_OUT_INLINE, FORWARD_OUT_COMMIT_CHAIN_VER = 1, 2, 4
FORWARD_RETURN, FORWARD_SEND, FORWARD_NO_SUCCESSOR, FORWARD_COMMIT = 1, 2, 3, 4
FORWARD_INFO_WORDS = 8
FORWARD_INFO_NAMES = ("sent", "returned", "no_successor", "sync_hashed", "sync_mismatched", "bad_records",
                      "reserved6", "reserved7")
FORWARD_DONE_NAMES = ("commits", "returned", "e7015", "e4081", "e4082", "rehashed", "corrupted", "unhashable")


class ServerReadJob(ctypes.Structure):
    """hf3fs_crc_server_read_job: one ReadIO of the server's batchRead around its AIO
    (StorageOperator.cc:98-226, BatchReadJob.cc:16-113, AioStatus.cc:27-55)."""
    _fields_ = [
        ("remote_addr", _u64c), ("inner_offset", _u64c), ("localbuf", _u64c), ("res", ctypes.c_int64),
        ("read_offset", _u64c), ("inline_off", _u64c),
        ("offset", _u32c), ("length", _u32c), ("rdmabuf_size", _u32c), ("rkey", _u32c),
        ("target_status", _i32c), ("meta_status", _i32c), ("commit_ver", _u32c), ("update_ver", _u32c),
        ("chain_ver", _u32c), ("chunk_len", _u32c), ("chunk_checksum", _u32c),
        ("meta_status_now", _i32c), ("update_ver_now", _u32c),
        # out of prepare
        ("head_len", _u32c), ("tail_len", _u32c), ("read_len", _u32c), ("buf_ordinal", _u32c), ("buf_off", _u32c),
        ("status", _i32c),
        # out of complete
        ("result_len", _u32c), ("result_status", _i32c), ("checksum", _u32c),
        ("has_rkey", _u8c), ("up_to_date", _u8c), ("engine", _u8c), ("chunk_checksum_type", _u8c),
        ("buf_kind", _u8c), ("checksum_type", _u8c), ("reserved", _u8c * 50),
    ]


class ServerReadReq(ctypes.Structure):
    """hf3fs_crc_server_read_req: one BatchReadReq; it owns a contiguous range of the jobs."""
    _fields_ = [
        ("total_len", _u64c), ("total_head", _u64c), ("total_tail", _u64c),
        ("inline_off", _u64c), ("inline_bytes", _u64c), ("wr_bytes", _u64c),
        ("max_msg_sz", _u32c), ("status", _i32c), ("failed_job", _u32c), ("n_small", _u32c), ("n_big", _u32c),
        ("n_ok", _u32c), ("wr_first", _u32c), ("wr_count", _u32c), ("wr_fails", _u32c),
        ("checksum_type", _u8c), ("xmit", _u8c), ("read_uncommitted", _u8c), ("recalculate", _u8c),
        ("reserved", _u8c * 40),
    ]


class ServerReadWr(ctypes.Structure):
    """hf3fs_crc_server_read_wr: one RDMA write of the list (RDMAReqBatch::add's arguments)."""
    _fields_ = [("remote_addr", _u64c), ("local_addr", _u64c), ("length", _u32c), ("rkey", _u32c), ("job", _u32c),
                ("req", _u32c)]


assert ctypes.sizeof(ServerReadJob) == 192 and ctypes.sizeof(ServerReadReq) == 128
assert ctypes.sizeof(ServerReadWr) == 32
RDMA_NO_BUF, CHUNK_METADATA_NOT_FOUND, CHUNK_METADATA_GET_ERROR, CHUNK_NOT_COMMIT = 2019, 4001, 4002, 4004
TARGET_STATE_INVALID = 4032
SERVER_READ_XMIT_RDMA, SERVER_READ_XMIT_INLINE, SERVER_READ_XMIT_NONE = 0, 1, 2
SERVER_READ_BUF_NONE, SERVER_READ_BUF_SMALL, SERVER_READ_BUF_BIG = 0, 1, 2
SERVER_READ_NONE = 0xFFFFFFFF  # ServerReadReq.failed_job: no job failed the request
SERVER_READ_INFO_WORDS = 8
SERVER_READ_INFO_NAMES = ("reqs_ok", "reqs_failed", "jobs_ok", "jobs_failed", "small", "big", "reserved6",
                          "reserved7")
SERVER_READ_DONE_NAMES = ("ok", "failed", "inline_lo", "inline_hi", "inline_overflow", "wr", "wr_fails", "hashed")


class ScrubIO(ctypes.Structure):
    """hf3fs_crc_scrub_io: one stored chunk vs its persisted checksum."""
    _fields_ = [
        ("data", ctypes.c_uint64),
        ("length", ctypes.c_uint32),
        ("checksum_type", ctypes.c_uint8),
        ("fin", ctypes.c_uint8),
        ("reserved", ctypes.c_uint16),
        ("checksum", ctypes.c_uint32),
        ("computed", ctypes.c_uint32),
        ("status", ctypes.c_int32),
        ("reserved2", ctypes.c_uint32),
    ]


class SyncMeta(ctypes.Structure):
    """hf3fs_crc_sync_meta: one chunk's metadata in the local or the remote table of a resync plan."""
    _fields_ = [
        ("id_hi", ctypes.c_uint64),
        ("id_lo", ctypes.c_uint64),
        ("chain_ver", ctypes.c_uint32),
        ("update_ver", ctypes.c_uint32),
        ("commit_ver", ctypes.c_uint32),
        ("checksum", ctypes.c_uint32),
        ("length", ctypes.c_uint32),
        ("chunk_size", ctypes.c_uint32),
        ("chunk_state", ctypes.c_uint8),
        ("recycle_state", ctypes.c_uint8),
        ("checksum_type", ctypes.c_uint8),
        ("out_class", ctypes.c_uint8),
        ("out_peer", ctypes.c_uint32),
    ]


assert ctypes.sizeof(SyncMeta) == 48
# SyncMeta.out_class (HF3FS_SYNC_*): remote records 1-12, local records 16-18
(SYNC_REMOTE_ONLY, SYNC_LOCAL_RECYCLING, SYNC_CHAIN_VER_LOW, SYNC_REMOTE_UNCOMMITTED, SYNC_REMOTE_CHAIN_VER_HIGH,
 SYNC_LOCAL_UNCOMMITTED, SYNC_COMMIT_VER_MISMATCH, SYNC_CHAIN_WRITING, SYNC_FULL_SYNC_HEAVY, SYNC_CHECKSUM_MISMATCH,
 SYNC_CHAIN_WRITING_CHECKSUM, SYNC_EQUAL) = range(1, 13)
SYNC_MATCHED, SYNC_REMOTE_MISS, SYNC_DUPLICATE = 16, 17, 18
SYNC_HEAVY = 1  # hf3fs_crc_sync_plan flags
SYNC_NONE = 0xFFFFFFFF  # no peer / no fatal record
SYNC_INFO_WORDS = 16
# words of d_info (HF3FS_SYNC_INFO_*), in order
SYNC_INFO_NAMES = ("fatal", "first_fatal", "n_write", "n_remove", "recycle", "chain_ver_low", "remote_uncommitted",
                   "chain_ver_high", "local_uncommitted", "commit_ver_mismatch", "chain_writing", "full_sync_heavy",
                   "full_sync_light", "skip", "remote_miss", "duplicates")


class RangeOp(ctypes.Structure):
    """hf3fs_crc_range_op: one QueryLastChunkOp or RemoveChunksOp payload, a walk over one target's
    chunk metadata by chunk-id range (StorageOperator.cc:653-751,858-1000)."""
    _fields_ = [
        ("begin_hi", _u64c), ("begin_lo", _u64c), ("end_hi", _u64c), ("end_lo", _u64c),
        ("max_chunks", _u32c), ("status_in", _i32c), ("kind", _u8c), ("reserved0", _u8c * 3), ("chain_id", _u32c),
        # out
        ("last_hi", _u64c), ("last_lo", _u64c), ("total_len", _u64c),
        ("total_chunks", _u32c), ("last_len", _u32c), ("last_index", _u32c), ("list_first", _u32c),
        ("status", _i32c), ("more", _u8c), ("reserved1", _u8c * 3),
    ]


class FileLen(ctypes.Structure):
    """hf3fs_crc_file_len: one file of the meta service's length fold (FileOperation.cc:45-179)."""
    _fields_ = [
        ("inode", _u64c), ("first_op", _u32c), ("n_file_ops", _u32c), ("chunk_size", _u32c), ("stripe_size", _u32c),
        ("flags", _u8c), ("reserved", _u8c * 3),
        # out
        ("status", _i32c), ("length", _u64c), ("total_len", _u64c), ("total_chunks", _u64c),
        ("last_chunk", _u32c), ("last_chunk_len", _u32c),
    ]


assert ctypes.sizeof(RangeOp) == 96 and ctypes.sizeof(FileLen) == 64
RANGE_QUERY, RANGE_REMOVE = 1, 2  # RangeOp.kind
RANGE_NONE = 0xFFFFFFFF  # RangeOp.last_index: no chunk; a saturated list_first
RANGE_INFO_WORDS = 8
RANGE_INFO_NAMES = ("ops_ok", "ops_failed", "chunks_lo", "chunks_hi", "list_lo", "list_hi", "list_overflow",
                    "unsorted")
RANGE_MAX_COUNT = 1 << 30
FILE_LEN_DYN = 1  # FileLen.flags
FILE_LEN_MAX_OPS = 1024
FILE_LEN_INFO_WORDS = 8
FILE_LEN_INFO_NAMES = ("ok", "failed", "empty", "not_found", "busy", "corrupt", "reserved6", "reserved7")
DATA_CORRUPTION, META_BUSY = 2, 3019  # StatusCode::kDataCorruption, MetaCode::kBusy


class Frame(ctypes.Structure):
    """hf3fs_crc_frame: one serde message of a receive buffer."""
    _fields_ = [
        ("offset", ctypes.c_uint64),
        ("size", ctypes.c_uint32),
        ("checksum", ctypes.c_uint32),
        ("computed", ctypes.c_uint32),
        ("status", ctypes.c_int32),
    ]


class EngineMeta(ctypes.Structure):
    """hf3fs_crc_engine_meta: the chunk engine's ChunkMeta (chunk_meta.rs:7-20)."""
    _fields_ = [
        ("pos", ctypes.c_uint64),
        ("chain_ver", ctypes.c_uint32),
        ("chunk_ver", ctypes.c_uint32),
        ("len", ctypes.c_uint32),
        ("checksum", ctypes.c_uint32),
        ("timestamp", ctypes.c_uint64),
        ("last_request_id", ctypes.c_uint64),
        ("last_client_low", ctypes.c_uint64),
        ("last_client_high", ctypes.c_uint64),
        ("etag_len", ctypes.c_uint8),
        ("uncommitted", ctypes.c_uint8),
        ("etag", ctypes.c_uint8 * 62),
    ]


assert ctypes.sizeof(ScrubIO) == 32 and ctypes.sizeof(Frame) == 24 and ctypes.sizeof(EngineMeta) == 120


class Anomaly(ctypes.Structure):
    """hf3fs_crc_anomaly: the update self-check's record."""
    _fields_ = [
        ("count", ctypes.c_uint32),
        ("kinds", ctypes.c_uint32),
        ("kind", ctypes.c_uint32),
        ("pipeline", ctypes.c_uint32),
        ("io", ctypes.c_uint64),
        ("pipeline_hash", ctypes.c_uint32),
        ("rehash", ctypes.c_uint32),
        ("client_checksum", ctypes.c_uint32),
        ("pre_max", ctypes.c_uint32),
        ("pre_addr", ctypes.c_uint64),
        ("pre_len", ctypes.c_uint64),
        ("payload", ctypes.c_uint64),
        ("length", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert ctypes.sizeof(Anomaly) == 72
ANOMALY_PAYLOAD_HASH, ANOMALY_PRE_JOB, ANOMALY_PRE_MAX, ANOMALY_START_ONLY, ANOMALY_RUN_COVER = 1, 2, 4, 8, 16


class CoalescerOptions(ctypes.Structure):
    """hf3fs_crc_coalescer_options (include/hf3fs_crc.h)."""
    _fields_ = [
        ("device", ctypes.c_int),
        ("max_batch", ctypes.c_uint32),
        ("max_wait_us", ctypes.c_uint32),
        ("slots", ctypes.c_uint32),
        ("inflight", ctypes.c_uint32),
        ("service_wgs", ctypes.c_uint32),
        ("stage_bytes", ctypes.c_uint64),
        ("service_ring", ctypes.c_uint32),
        ("service_idle_us", ctypes.c_uint32),
        ("service_stage", ctypes.c_uint64),
    ]


assert ctypes.sizeof(CoalescerOptions) == 48
REQ_HOST_COPY = 1
DONE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32)

_vp, _u8, _u32, _u64, _int = ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
SIGNATURES = {
    "hf3fs_crc_init": (_int, [_int]),
    "hf3fs_crc_shutdown": (None, []),
    "hf3fs_crc_last_error": (ctypes.c_char_p, []),
    "hf3fs_crc_version": (ctypes.c_char_p, []),
    "hf3fs_crc32c_combine": (_u32, [_u32, _u32, _u64]),
    "hf3fs_crc32_combine": (_u32, [_u32, _u32, _u64]),
    "hf3fs_crc_shift": (_u32, [_u8, _u32, _u64]),
    "hf3fs_checksum_combine": (_int, [ctypes.POINTER(_u8), ctypes.POINTER(_u32), _u8, _u32, _u64]),
    "hf3fs_crc_create_batch": (_int, [_u8, _vp, _vp, _vp, _vp, _u64, _u64, _vp]),
    "hf3fs_crc_create_strided": (_int, [_u8, _vp, _u64, _u64, _u64, _u32, _vp, _vp]),
    "hf3fs_crc_verify_batch": (_int, [_u8, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _vp]),
    "hf3fs_crc_verify_strided": (_int, [_u8, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    "hf3fs_crc_verify_blocks": (_int, [_u8, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp]),
    "hf3fs_crc_combine_batch": (_int, [_u8, _vp, _vp, _vp, _u64, _vp]),
    "hf3fs_crc_update_batch": (_int, [_u8, _vp, _u64, _u32, _int, _vp]),
    "hf3fs_crc_update_scratch_bytes": (ctypes.c_size_t, [_u64, _int]),
    "hf3fs_crc_update_ordered": (_int, [_u8, _vp, _u64, _u32, _int, _u32, _vp, _vp]),
    "hf3fs_crc_update_ordered_scratch_bytes": (ctypes.c_size_t, [_u64, _u32, _int, _u32]),
    "hf3fs_crc_update_versioned": (_int, [_u8, _vp, _vp, _u64, _u32, _int, _u32, _vp, _vp]),
    "hf3fs_crc_update_versioned_scratch_bytes": (ctypes.c_size_t, [_u64, _u32, _int, _u32]),
    "hf3fs_crc_update_engine": (_int, [_u8, _vp, _vp, _u64, _u32, _int, _u32, _vp, _vp]),
    "hf3fs_crc_update_engine_scratch_bytes": (ctypes.c_size_t, [_u64, _u32, _int, _u32]),
    "hf3fs_crc_update_cow_batch": (_int, [_u8, _vp, _vp, _u64, _u32, _int, _vp]),
    "hf3fs_crc_update_cow_scratch_bytes": (ctypes.c_size_t, [_u64, _u32, _int]),
    "hf3fs_crc_pair_scratch_stats": (_int, [_vp, _vp, _vp]),
    "hf3fs_crc_read_result_batch": (_int, [_u8, _vp, _u64, _u32, _vp]),
    "hf3fs_crc_client_read_batch": (_int, [_u8, _vp, _u64, _vp, _u64, _u64, _u32, _u32, _vp, _vp, _vp, _vp]),
    "hf3fs_crc_client_read_scratch_bytes": (ctypes.c_size_t, [_u64, _u64]),
    "hf3fs_crc_client_write_prepare": (_int, [_u8, _vp, _u64, _u32, _u32, _u32, _vp, _vp, _vp]),
    "hf3fs_crc_client_write_complete": (_int, [_vp, _u64, _vp, _u64, _u64, _u32, _vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "hf3fs_crc_client_write_scratch_bytes": (ctypes.c_size_t, [_u64, _u64]),
    "hf3fs_crc_forward_prepare": (_int, [_u8, _vp, _u64, _u32, _u32, _vp, _vp]),
    "hf3fs_crc_forward_complete": (_int, [_u8, _vp, _u64, _u32, _vp, _vp, _vp]),
    "hf3fs_crc_forward_scratch_bytes": (ctypes.c_size_t, [_u64]),
    "hf3fs_crc_server_read_prepare": (_int, [_vp, _u64, _vp, _vp, _u64, _u64, _u32, _u32, _vp, _vp]),
    "hf3fs_crc_server_read_complete": (_int, [_u8, _vp, _u64, _vp, _vp, _u64, _u32, _vp, _u64, _vp, _u64, _vp, _vp]),
    "hf3fs_crc_server_read_scratch_bytes": (ctypes.c_size_t, [_u64, _u64]),
    "hf3fs_crc_range_query": (_int, [_vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp]),
    "hf3fs_crc_range_query_scratch_bytes": (ctypes.c_size_t, [_u64, _u64]),
    "hf3fs_crc_file_length": (_int, [_vp, _u64, _vp, _u64, _vp, _vp]),
    "hf3fs_crc_file_digest_batch": (_int, [_vp, _vp, _vp, _u64, _u64, _vp]),
    "hf3fs_crc_file_digest_batch_ex": (_int, [_vp, _vp, _vp, _u64, _u64, _u32, _vp]),
    "hf3fs_crc_md5_batch": (_int, [_vp, _vp, _u64, _u64, _vp, _vp, _u32, _vp]),
    "hf3fs_crc_md5_scratch_bytes": (ctypes.c_size_t, [_u64]),
    "hf3fs_crc_md5_hex": (_u32, [_vp, _vp]),
    "hf3fs_crc_create_host": (_int, [_u8, _vp, _vp, _vp, _vp, _u64]),
    "hf3fs_crc_fill_synth": (_int, [_vp, _u64, _u64, _u64, _u64, _u64, _vp]),
    "hf3fs_crc_scrub_batch": (_int, [_u8, _vp, _u64, _u32, _vp, _vp]),
    "hf3fs_crc_sync_plan": (_int, [_vp, _u64, _vp, _u64, _u32, _u32, _vp, _vp, _vp, _vp]),
    "hf3fs_crc_sync_plan_scratch_bytes": (ctypes.c_size_t, [_u64, _u64]),
    "hf3fs_crc_sync_scrub_fill": (_int, [_vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "hf3fs_crc_engine_meta_decode": (_int, [_vp, _u64, ctypes.POINTER(EngineMeta), ctypes.POINTER(_u64)]),
    "hf3fs_crc_engine_meta_encode": (_int, [ctypes.POINTER(EngineMeta), _vp, _u64, ctypes.POINTER(_u64)]),
    "hf3fs_crc_default_etag": (_u32, [_u32, _vp]),
    "hf3fs_crc_frame_walk": (_int, [_vp, _u64, _vp, _u64, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    "hf3fs_crc_frame_verify_batch": (_int, [_vp, _vp, _u64, _u32, _vp, _vp]),
    "hf3fs_crc_coalescer_default_options": (None, [ctypes.POINTER(CoalescerOptions)]),
    "hf3fs_crc_coalescer_create": (_int, [ctypes.POINTER(CoalescerOptions), ctypes.POINTER(_vp)]),
    "hf3fs_crc_coalescer_destroy": (None, [_vp]),
    "hf3fs_crc_coalescer_submit": (_int, [_vp, _u8, _vp, _u64, _u32, _u32, DONE_FN, _vp]),
    "hf3fs_crc_coalescer_create_one": (_int, [_vp, _u8, _vp, _u64, _u32, _u32, ctypes.POINTER(_u32)]),
    "hf3fs_crc_coalescer_stats": (_int, [_vp, ctypes.POINTER(_u64)]),
    "hf3fs_crc_host_register": (_int, [_vp, _u64, ctypes.POINTER(_vp)]),
    "hf3fs_crc_host_unregister": (_int, [_vp]),
    "hf3fs_checksum_serialize": (_u32, [_u8, _u32, _vp]),
    "hf3fs_checksum_deserialize": (_int, [_vp, _u64, ctypes.POINTER(_u8), ctypes.POINTER(_u32), ctypes.POINTER(_u64)]),
    "hf3fs_crc_serialize_batch": (_int, [_u8, _vp, _u64, _vp, _vp]),
    "hf3fs_crc_finalize_batch": (_int, [_vp, _u64, _vp]),
    "hf3fs_crc32c_combine_fin": (_u32, [_u32, _u32, _u64]),
    "hf3fs_crc_release_stream": (_int, [_vp]),
    "hf3fs_crc_release_graph_scratch": (_int, []),
    "hf3fs_crc_graph_scratch_stats": (_int, [_vp, _vp, _vp]),
    "hf3fs_crc_stream_wait": (_int, [_vp, _u32]),
    "hf3fs_crc_set_option": (_int, [ctypes.c_char_p, ctypes.c_char_p]),
    "hf3fs_crc_get_option": (_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]),
    "hf3fs_crc_anomalies": (_int, [_int, ctypes.c_void_p, _int]),
}

_lib = None


def header_symbols():
    """Function names declared in include/hf3fs_crc.h."""
    text = open(HEADER).read()
    return sorted(set(re.findall(r"\b(hf3fs_[a-z0-9_]+)\s*\(", text)))


def load():
    """Load the HIP library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} missing: run `python 3fs_amd/build.py` (hipcc --offload-arch=gfx950)")
    L = ctypes.CDLL(LIB_PATH)
    ab_build = bool(os.environ.get("HF3FS_CRC_LIB"))  # an A/B build may predate newer entry points
    for name, (res, args) in SIGNATURES.items():
        if ab_build and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def check(rc):
    if rc != OK:
        msg = load().hf3fs_crc_last_error()
        raise Hf3fsCrcError(rc, msg.decode() if msg else "")
    return rc


def _p(x):
    """Device/host address of a torch tensor, an int, or None."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    return x.data_ptr()


def _s(stream):
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream


# ---- thin wrappers (addresses may be torch tensors or ints) ------------------
def create_strided(ctype, base, stride, length, n, out, start=0xFFFFFFFF, stream=None):
    return check(load().hf3fs_crc_create_strided(ctype, _p(base), stride, length, n, start, _p(out), _s(stream)))


def create_batch(ctype, bufs, lens, out, n, max_len, starts=None, stream=None):
    return check(load().hf3fs_crc_create_batch(ctype, _p(bufs), _p(lens), _p(starts), _p(out), n, max_len,
                                               _s(stream)))


def verify_batch(ctype, bufs, lens, expected, mismatch, count, n, max_len, computed=None, stream=None):
    return check(load().hf3fs_crc_verify_batch(ctype, _p(bufs), _p(lens), _p(expected), _p(mismatch), _p(count),
                                               _p(computed), n, max_len, _s(stream)))


def verify_strided(ctype, base, stride, length, n, expected, mismatch, count, computed=None, stream=None):
    return check(load().hf3fs_crc_verify_strided(ctype, _p(base), stride, length, n, _p(expected), _p(mismatch),
                                                 _p(count), _p(computed), _s(stream)))


def verify_blocks(ctype, arena, offsets, lens, expected, mismatch, count, n, max_len, computed=None, stream=None):
    return check(load().hf3fs_crc_verify_blocks(ctype, _p(arena), _p(offsets), _p(lens), _p(expected),
                                                _p(mismatch), _p(count), _p(computed), n, max_len, _s(stream)))


def combine_batch(ctype, acc, crc2, len2, n, stream=None):
    return check(load().hf3fs_crc_combine_batch(ctype, _p(acc), _p(crc2), _p(len2), n, _s(stream)))


def update_batch(ctype, ios, n, max_len, mode=MODE_REFERENCE, stream=None):
    """hf3fs_crc_update_batch; REFERENCE by default (DELTA trusts the stored checksum)."""
    return check(load().hf3fs_crc_update_batch(ctype, _p(ios), n, max_len, mode, _s(stream)))


def update_scratch_bytes(n, mode=MODE_REFERENCE):
    """Bytes of library-owned scratch one update_batch of n IOs takes (the calling
    (stream, thread) pair's buffer, or a captured call's own; never the stream-ordered pool)."""
    return int(load().hf3fs_crc_update_scratch_bytes(n, mode))


def update_ordered(ctype, ios, n, max_len, max_rounds, mode=MODE_REFERENCE, info=None, stream=None):
    """hf3fs_crc_update_ordered: n IOs in arrival order, chunks may repeat (at most max_rounds IOs
    per chunk are applied, the rest come back NOT_APPLIED); info: two device u32 words or None."""
    return check(load().hf3fs_crc_update_ordered(ctype, _p(ios), n, max_len, mode, max_rounds, _p(info), _s(stream)))


def update_ordered_scratch_bytes(n, max_len, max_rounds, mode=MODE_REFERENCE):
    """Bytes of library-owned scratch one update_ordered of this shape takes (0: rejected arguments)."""
    return int(load().hf3fs_crc_update_ordered_scratch_bytes(n, max_len, mode, max_rounds))


def update_versioned(ctype, ios, ver, n, max_len, max_rounds, mode=MODE_REFERENCE, info=None, stream=None):
    """hf3fs_crc_update_versioned: update_ordered with the reference's version ladder and commit jobs.
    ver: a device array of n hf3fs_crc_update_ver (update_ver_dtype()) parallel to ios, or None (the
    call is then update_ordered); info: VER_INFO_WORDS device u32 words or None."""
    return check(load().hf3fs_crc_update_versioned(ctype, _p(ios), _p(ver), n, max_len, mode, max_rounds, _p(info),
                                                   _s(stream)))


def update_versioned_scratch_bytes(n, max_len, max_rounds, mode=MODE_REFERENCE):
    """Bytes of library-owned scratch one update_versioned with version records takes (0: rejected)."""
    return int(load().hf3fs_crc_update_versioned_scratch_bytes(n, max_len, mode, max_rounds))


def update_engine(ctype, ios, jobs, n, max_len, max_rounds, mode=MODE_REFERENCE, info=None, stream=None):
    """hf3fs_crc_update_engine: a chunk-engine target's queue of update and commit jobs in arrival
    order.  jobs: a device array of n hf3fs_crc_engine_job (engine_job_dtype()) parallel to ios;
    info: ENGINE_INFO_WORDS device u32 words or None."""
    return check(load().hf3fs_crc_update_engine(ctype, _p(ios), _p(jobs), n, max_len, mode, max_rounds, _p(info),
                                                _s(stream)))


def update_engine_scratch_bytes(n, max_len, max_rounds, mode=MODE_REFERENCE):
    """Bytes of library-owned scratch one update_engine of this shape takes (0: rejected arguments)."""
    return int(load().hf3fs_crc_update_engine_scratch_bytes(n, max_len, mode, max_rounds))


def update_cow(ctype, ios, dst, n, max_len, mode=MODE_REFERENCE, stream=None):
    """hf3fs_crc_update_cow_batch: update_batch with a device array of n destination addresses
    (None: every IO in place; entry 0 or the IO's chunk: that IO in place)."""
    return check(load().hf3fs_crc_update_cow_batch(ctype, _p(ios), _p(dst), n, max_len, mode, _s(stream)))


def update_cow_scratch_bytes(n, max_len, mode=MODE_REFERENCE):
    """Bytes of library-owned scratch one update_cow_batch of this shape takes (0: rejected arguments)."""
    return int(load().hf3fs_crc_update_cow_scratch_bytes(n, max_len, mode))


def pair_scratch_stats(stream=None):
    """{call_bytes, allocations}: the calling (stream, thread) pair's call scratch and the
    process's count of pair-buffer allocations and growths (test aid)."""
    v = (ctypes.c_uint64 * 2)()
    check(load().hf3fs_crc_pair_scratch_stats(_s(stream), ctypes.addressof(v), ctypes.addressof(v) + 8))
    return {"call_bytes": int(v[0]), "allocations": int(v[1])}


def set_option(name, value):
    """hf3fs_crc_set_option: a tuning / test switch for every later call."""
    return check(load().hf3fs_crc_set_option(name.encode(), str(value).encode()))


def get_option(name):
    out = ctypes.create_string_buffer(32)
    check(load().hf3fs_crc_get_option(name.encode(), out, 32))
    return out.value.decode()


class option:
    """with option("update_pipeline", "fused"): ... -- set for the block, restored after."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = get_option(self.name)
        set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.old)


def anomalies(device=0, reset=False):
    """hf3fs_crc_anomalies: the update self-check's record as a dict (device-synchronizes)."""
    a = Anomaly()
    check(load().hf3fs_crc_anomalies(device, ctypes.byref(a), 1 if reset else 0))
    return a.as_dict()


def release_stream(stream):
    return check(load().hf3fs_crc_release_stream(_s(stream)))


def release_graph_scratch():
    return check(load().hf3fs_crc_release_graph_scratch())


def stream_wait(stream=None, poll_us=20):
    """Wait for the stream's queued work, polling with a poll_us sleep (0: hipStreamSynchronize)."""
    return check(load().hf3fs_crc_stream_wait(_s(stream), poll_us))


def graph_scratch_stats():
    """{live, live_bytes, dead}: buffers of captured calls still owned by a graph, and
    those whose graph is gone, awaiting the next uncaptured call's free."""
    v = (ctypes.c_uint64 * 3)()
    check(load().hf3fs_crc_graph_scratch_stats(ctypes.addressof(v), ctypes.addressof(v) + 8, ctypes.addressof(v) + 16))
    return {"live": int(v[0]), "live_bytes": int(v[1]), "dead": int(v[2])}


def read_result_batch(ctype, ios, n, max_len, stream=None):
    return check(load().hf3fs_crc_read_result_batch(ctype, _p(ios), n, max_len, _s(stream)))


def file_digest_batch(blocks, file_off, out, n_files, max_blocks, stream=None, fill_zero=True):
    """blocks: device array of hf3fs_crc_block_digest; file_off: n_files+1 uint64;
    out: n_files hf3fs_crc_file_digest (see include/hf3fs_crc.h).  fill_zero=False:
    the admin command without --fill-zero (first missing / short block is the status)."""
    return check(load().hf3fs_crc_file_digest_batch_ex(_p(blocks), _p(file_off), _p(out), n_files, max_blocks,
                                                       DIGEST_FILL_ZERO if fill_zero else 0, _s(stream)))


def client_read_io_dtype():
    """numpy dtype of hf3fs_crc_client_read_io (include/hf3fs_crc.h): one 40-byte record per IO."""
    import numpy as np
    return np.dtype([("data", "<u8"), ("length", "<u4"), ("read_len", "<u4"), ("status_in", "<i4"),
                     ("checksum", "<u4"), ("checksum_type", "u1"), ("reserved0", "u1", (3,)), ("computed", "<u4"),
                     ("status", "<i4"), ("reserved1", "<u4")])


def client_read_result_dtype():
    """numpy dtype of hf3fs_crc_client_read_result: one 24-byte record per parent."""
    import numpy as np
    return np.dtype([("length", "<u4"), ("checksum", "<u4"), ("checksum_type", "u1"), ("reserved", "u1", (3,)),
                     ("status", "<i4"), ("failed_child", "<u4"), ("block_len", "<u4")])


def block_digest_dtype():
    """numpy dtype of hf3fs_crc_block_digest: what client_read_batch hands to file_digest_batch."""
    import numpy as np
    return np.dtype([("read_len", "<u8"), ("block_len", "<u8"), ("checksum", "<u4"), ("checksum_type", "u1"),
                     ("missing", "u1"), ("reserved", "u1", (2,))])


def client_read_batch(ctype, ios, n_ios, info, parent_off=None, n_parents=None, max_children=1, max_len=0,
                      verify=True, parents=None, blocks=None, flags=None, stream=None):
    """hf3fs_crc_client_read_batch: ios a device array of hf3fs_crc_client_read_io (computed and
    status updated in place), parent_off n_parents + 1 device uint64 or None (every IO its own
    parent), parents / blocks device arrays of hf3fs_crc_client_read_result / hf3fs_crc_block_digest
    (either may be None), info CLIENT_READ_INFO_WORDS device u32.  flags overrides verify."""
    if n_parents is None:
        n_parents = n_ios
    if flags is None:
        flags = CLIENT_READ_VERIFY if verify else 0
    return check(load().hf3fs_crc_client_read_batch(ctype, _p(ios), n_ios, _p(parent_off), n_parents, max_children,
                                                    max_len, flags, _p(parents), _p(blocks), _p(info), _s(stream)))


def client_read_scratch_bytes(n_ios, n_parents):
    """Bytes of library-owned scratch one verifying client_read_batch takes (0: rejected counts)."""
    return int(load().hf3fs_crc_client_read_scratch_bytes(n_ios, n_parents))


def _dtype_of(struct):
    import numpy as np
    kinds = {_u8c: "u1", _u32c: "<u4", _i32c: "<i4", _u64c: "<u8"}
    return np.dtype([(name, kinds[t]) if t in kinds else (name, "u1", (ctypes.sizeof(t),))
                     for name, t in struct._fields_])


def client_write_io_dtype():
    """numpy dtype of hf3fs_crc_client_write_io (include/hf3fs_crc.h): one 64-byte record per IO."""
    return _dtype_of(ClientWriteIO)


def client_write_file_dtype():
    """numpy dtype of hf3fs_crc_client_write_file: one 24-byte record per file."""
    return _dtype_of(ClientWriteFile)


def update_io_dtype():
    """numpy dtype of hf3fs_crc_update_io: the 56-byte record client_write_prepare fills the request of."""
    return _dtype_of(UpdateIO)


def client_write_prepare(ctype, ios, n, info, max_len, max_inline_bytes=0, verify=True, updates=None, flags=None,
                         stream=None):
    """hf3fs_crc_client_write_prepare: ios a device array of hf3fs_crc_client_write_io (checksum,
    checksum_type, send_inline and status written in place), updates a device array of
    hf3fs_crc_update_io or None, info CLIENT_WRITE_INFO_WORDS device u32.  flags overrides verify."""
    if flags is None:
        flags = CLIENT_WRITE_VERIFY if verify else 0
    return check(load().hf3fs_crc_client_write_prepare(ctype, _p(ios), n, max_len, max_inline_bytes, flags,
                                                       _p(updates), _p(info), _s(stream)))


def client_write_complete(ios, n, info, file_off=None, n_files=0, max_ios_per_file=1, updates=None, expected=None,
                          files=None, failed=None, failed_cap=0, flags=None, stream=None):
    """hf3fs_crc_client_write_complete: file_off n_files + 1 device uint64, expected n_files device
    u32 or None, files a device array of hf3fs_crc_client_write_file, failed failed_cap device u32,
    info CLIENT_WRITE_DONE_WORDS device u32.  flags defaults to FROM_UPDATES when updates is given."""
    if flags is None:
        flags = CLIENT_WRITE_FROM_UPDATES if updates is not None else 0
    return check(load().hf3fs_crc_client_write_complete(_p(ios), n, _p(file_off), n_files, max_ios_per_file, flags,
                                                        _p(updates), _p(expected), _p(files), _p(failed), failed_cap,
                                                        _p(info), _s(stream)))


def client_write_scratch_bytes(n, n_files=0):
    """Bytes of library-owned scratch either client_write call takes for n IOs (0: rejected counts)."""
    return int(load().hf3fs_crc_client_write_scratch_bytes(n, n_files))


def forward_job_dtype():
    """numpy dtype of hf3fs_crc_forward_job (include/hf3fs_crc.h): one 192-byte record per job."""
    import numpy as np
    kinds = {_u8c: "u1", _u32c: "<u4", _i32c: "<i4", _u64c: "<u8"}
    return np.dtype([(name, kinds[t]) if t in kinds else (name, "u1", (ctypes.sizeof(t),))
                     for name, t in ForwardJob._fields_])


def forward_prepare(ctype, jobs, n, info, max_len, max_inline_bytes=0, stream=None):
    """hf3fs_crc_forward_prepare: jobs a device array of hf3fs_crc_forward_job (the prepare outputs
    written in place), info FORWARD_INFO_WORDS device u32."""
    return check(load().hf3fs_crc_forward_prepare(ctype, _p(jobs), n, max_len, max_inline_bytes, _p(info),
                                                  _s(stream)))


def forward_complete(ctype, jobs, n, info, max_len, commit_idx=None, stream=None):
    """hf3fs_crc_forward_complete: the complete outputs written in place, commit_idx n device u32 or
    None (the COMMIT jobs' indices, ascending; their count is info[0])."""
    return check(load().hf3fs_crc_forward_complete(ctype, _p(jobs), n, max_len, _p(commit_idx), _p(info),
                                                   _s(stream)))


def forward_scratch_bytes(n):
    """Bytes of library-owned scratch either forward call takes for n jobs (0: rejected count)."""
    return int(load().hf3fs_crc_forward_scratch_bytes(n))


def _record_dtype(struct):
    import numpy as np
    kinds = {_u8c: "u1", _u32c: "<u4", _i32c: "<i4", _u64c: "<u8", ctypes.c_int64: "<i8"}
    return np.dtype([(name, kinds[t]) if t in kinds else (name, "u1", (ctypes.sizeof(t),))
                     for name, t in struct._fields_])


def server_read_job_dtype():
    """numpy dtype of hf3fs_crc_server_read_job (include/hf3fs_crc.h): one 192-byte record per ReadIO."""
    return _record_dtype(ServerReadJob)


def server_read_req_dtype():
    """numpy dtype of hf3fs_crc_server_read_req: one 128-byte record per BatchReadReq."""
    return _record_dtype(ServerReadReq)


def server_read_wr_dtype():
    """numpy dtype of hf3fs_crc_server_read_wr: one 32-byte entry of the RDMA write list."""
    return _record_dtype(ServerReadWr)


def server_read_prepare(jobs, n, reqs, req_off, n_reqs, info, small_buf, big_buf, max_jobs_per_req=0, stream=None):
    """hf3fs_crc_server_read_prepare: jobs / reqs device arrays of the two records (the prepare
    outputs written in place), req_off n_reqs + 1 device u64, info SERVER_READ_INFO_WORDS device u32."""
    return check(load().hf3fs_crc_server_read_prepare(_p(jobs), n, _p(reqs), _p(req_off), n_reqs, max_jobs_per_req,
                                                      small_buf, big_buf, _p(info), _s(stream)))


def server_read_complete(ctype, jobs, n, reqs, req_off, n_reqs, info, max_len, inline=None, inline_cap=0, wr=None,
                         wr_cap=0, stream=None):
    """hf3fs_crc_server_read_complete: the complete outputs written in place, inline the response
    arena of inline_cap bytes or None, wr wr_cap device hf3fs_crc_server_read_wr or None."""
    return check(load().hf3fs_crc_server_read_complete(ctype, _p(jobs), n, _p(reqs), _p(req_off), n_reqs, max_len,
                                                       _p(inline), inline_cap, _p(wr), wr_cap, _p(info), _s(stream)))


def server_read_scratch_bytes(n, n_reqs=0):
    """Bytes of library-owned scratch complete takes for n jobs of n_reqs requests (0: rejected counts)."""
    return int(load().hf3fs_crc_server_read_scratch_bytes(n, n_reqs))


def range_op_dtype():
    """numpy dtype of hf3fs_crc_range_op: one 96-byte record per range walk."""
    return _record_dtype(RangeOp)


def file_len_dtype():
    """numpy dtype of hf3fs_crc_file_len: one 64-byte record per file."""
    return _record_dtype(FileLen)


def sync_meta_dtype():
    """numpy dtype of hf3fs_crc_sync_meta: the table record of sync_plan and range_query."""
    import numpy as np
    kinds = {ctypes.c_uint8: "u1", ctypes.c_uint32: "<u4", ctypes.c_uint64: "<u8"}
    return np.dtype([(name, kinds[t]) for name, t in SyncMeta._fields_])


def range_query(meta, n_meta, ops, n_ops, info, list_out=None, list_cap=0, stream=None):
    """hf3fs_crc_range_query: meta a device array of hf3fs_crc_sync_meta, strictly ascending by id
    (read only), ops a device array of hf3fs_crc_range_op (outputs written in place), list_out
    list_cap device u32 or None, info RANGE_INFO_WORDS device u32."""
    return check(load().hf3fs_crc_range_query(_p(meta), n_meta, _p(ops), n_ops, _p(list_out), list_cap, _p(info),
                                              _s(stream)))


def range_query_scratch_bytes(n_meta, n_ops):
    """Bytes of library-owned scratch one range_query of this shape takes (0: rejected counts)."""
    return int(load().hf3fs_crc_range_query_scratch_bytes(n_meta, n_ops))


def file_length(ops, n_ops, files, n_files, info, stream=None):
    """hf3fs_crc_file_length: ops finished range ops (read only), files a device array of
    hf3fs_crc_file_len (outputs written in place), info FILE_LEN_INFO_WORDS device u32."""
    return check(load().hf3fs_crc_file_length(_p(ops), n_ops, _p(files), n_files, _p(info), _s(stream)))


MD5_INIT, MD5_FINAL = 1, 2  # hf3fs_crc_md5_batch flags


def md5_seg_dtype():
    """numpy dtype of hf3fs_crc_md5_seg (include/hf3fs_crc.h): one 16-byte record per segment."""
    import numpy as np
    return np.dtype([("data", "<u8"), ("length", "<u8")])


def md5_state_dtype():
    """numpy dtype of hf3fs_crc_md5_state (include/hf3fs_crc.h): one 96-byte record per file."""
    import numpy as np
    return np.dtype([("h", "<u4", (4,)), ("total", "<u8"), ("tail", "u1", (64,)), ("reserved", "<u8")])


def md5_batch(segs, file_off, n_files, n_segs, out=None, state=None, flags=MD5_INIT | MD5_FINAL, stream=None):
    """hf3fs_crc_md5_batch: segs a device array of hf3fs_crc_md5_seg (md5_seg_dtype()), file_off
    n_files + 1 device uint64, out 16 n_files device bytes (FINAL), state a device array of
    hf3fs_crc_md5_state (md5_state_dtype()) or None (the one-shot form, INIT | FINAL)."""
    return check(load().hf3fs_crc_md5_batch(_p(segs), _p(file_off), n_files, n_segs, _p(state), _p(out), flags,
                                            _s(stream)))


def md5_scratch_bytes(n_files):
    """Bytes of library-owned scratch one md5_batch of n_files takes (0: a rejected count)."""
    return int(load().hf3fs_crc_md5_scratch_bytes(n_files))


def md5_hex(digest):
    """16 digest bytes -> the 32 lower-case hex characters the admin command prints."""
    b = bytes(digest)
    if len(b) != 16:
        raise ValueError("an MD5 digest has 16 bytes")
    src = ctypes.create_string_buffer(b, 16)
    out = ctypes.create_string_buffer(32)
    k = load().hf3fs_crc_md5_hex(src, out)
    return out.raw[:k].decode()


def scrub_batch(ctype, ios, n, max_len, count, stream=None):
    """ios: device array of hf3fs_crc_scrub_io (updated in place); count: device u32."""
    return check(load().hf3fs_crc_scrub_batch(ctype, _p(ios), n, max_len, _p(count), _s(stream)))


def sync_plan(local, n_local, remote, n_remote, chain_ver, info, write=None, remove=None, flags=0, stream=None):
    """hf3fs_crc_sync_plan: local / remote are device arrays of hf3fs_crc_sync_meta (out_class and
    out_peer updated in place), info SYNC_INFO_WORDS device u32, write / remove device u32 lists of
    capacity n_local / n_remote (either may be None)."""
    return check(load().hf3fs_crc_sync_plan(_p(local), n_local, _p(remote), n_remote, chain_ver, flags, _p(write),
                                            _p(remove), _p(info), _s(stream)))


def sync_plan_scratch_bytes(n_local, n_remote):
    """Bytes of library-owned scratch one sync_plan of this shape takes (0: rejected counts)."""
    return int(load().hf3fs_crc_sync_plan_scratch_bytes(n_local, n_remote))


def sync_scrub_fill(local, addrs, write, info, n_local, scrub, stream=None):
    """hf3fs_crc_sync_scrub_fill: n_local hf3fs_crc_scrub_io records from a plan's write list."""
    return check(load().hf3fs_crc_sync_scrub_fill(_p(local), _p(addrs), _p(write), _p(info), n_local, _p(scrub),
                                                  _s(stream)))


def frame_verify_batch(buf, frames, n, max_size, count, stream=None):
    return check(load().hf3fs_crc_frame_verify_batch(_p(buf), _p(frames), n, max_size, _p(count), _s(stream)))


def frame_walk(data, max_frames=None):
    """Processor::unpackMsg framing walk over host bytes -> (status, [Frame], consumed)."""
    b = bytes(data)
    cap = max_frames if max_frames is not None else max(1, len(b) // 8)
    frames = (Frame * max(1, cap))()
    nf, used = ctypes.c_uint64(), ctypes.c_uint64()
    buf = ctypes.create_string_buffer(b, max(1, len(b)))
    rc = load().hf3fs_crc_frame_walk(buf, len(b), frames, cap, ctypes.byref(nf), ctypes.byref(used))
    return rc, [frames[i] for i in range(nf.value)], int(used.value)


def engine_meta_decode(data):
    """derse ChunkMeta bytes -> (status, EngineMeta, consumed)."""
    b = bytes(data)
    m = EngineMeta()
    used = ctypes.c_uint64()
    buf = ctypes.create_string_buffer(b, max(1, len(b)))
    rc = load().hf3fs_crc_engine_meta_decode(buf, len(b), ctypes.byref(m), ctypes.byref(used))
    return rc, m, int(used.value)


def engine_meta_encode(m):
    out = ctypes.create_string_buffer(256)
    w = ctypes.c_uint64()
    rc = load().hf3fs_crc_engine_meta_encode(ctypes.byref(m), out, 256, ctypes.byref(w))
    return rc, out.raw[:w.value]


def default_etag(checksum_fin):
    out = ctypes.create_string_buffer(8)
    k = load().hf3fs_crc_default_etag(checksum_fin, out)
    return out.raw[:k].decode()


def fill_synth(dst, stride, chunk_len, n_chunks, seed, first_chunk_id=0, stream=None):
    return check(load().hf3fs_crc_fill_synth(_p(dst), stride, chunk_len, n_chunks, seed, first_chunk_id,
                                             _s(stream)))


def create_host(ctype, buffers, starts=None):
    """ChecksumInfo::create over a list of host bytes-like objects -> list of raw values."""
    n = len(buffers)
    keep = [ctypes.create_string_buffer(bytes(b), max(1, len(b))) for b in buffers]
    ptrs = (ctypes.c_void_p * max(1, n))(*[ctypes.addressof(k) for k in keep])
    lens = (ctypes.c_uint64 * max(1, n))(*[len(b) for b in buffers])
    st = (ctypes.c_uint32 * max(1, n))(*starts) if starts is not None else None
    out = (ctypes.c_uint32 * max(1, n))()
    check(load().hf3fs_crc_create_host(ctype, ptrs, lens, st, out, n))
    return [int(out[i]) for i in range(n)]


def checksum_serialize(ctype, value):
    """ChecksumInfo in serde binary form (6 bytes)."""
    out = ctypes.create_string_buffer(6)
    k = load().hf3fs_checksum_serialize(ctype, value, out)
    return out.raw[:k]


def checksum_deserialize(data):
    """-> (status, (type, value), consumed)."""
    b = bytes(data)
    t, v, used = ctypes.c_uint8(), ctypes.c_uint32(), ctypes.c_uint64()
    buf = ctypes.create_string_buffer(b, max(1, len(b)))
    rc = load().hf3fs_checksum_deserialize(buf, len(b), ctypes.byref(t), ctypes.byref(v), ctypes.byref(used))
    return rc, (int(t.value), int(v.value)), int(used.value)


def serialize_batch(ctype, values, n, out, stream=None):
    return check(load().hf3fs_crc_serialize_batch(ctype, _p(values), n, _p(out), _s(stream)))


def finalize_batch(values, n, stream=None):
    return check(load().hf3fs_crc_finalize_batch(_p(values), n, _s(stream)))


def crc32c_combine_fin(f1, f2, len2):
    return int(load().hf3fs_crc32c_combine_fin(f1, f2, len2))


def crc32c_combine(c1, c2, len2):
    return int(load().hf3fs_crc32c_combine(c1, c2, len2))


def crc32_combine(c1, c2, len2):
    return int(load().hf3fs_crc32_combine(c1, c2, len2))


def shift(ctype, crc, nbytes):
    return int(load().hf3fs_crc_shift(ctype, crc, nbytes))


def checksum_combine(a, b, length):
    """ChecksumInfo::combine on (type, value) tuples -> (status, (type, value))."""
    t = ctypes.c_uint8(a[0])
    v = ctypes.c_uint32(a[1])
    rc = load().hf3fs_checksum_combine(ctypes.byref(t), ctypes.byref(v), b[0], b[1], length)
    return rc, (int(t.value), int(v.value))


class Coalescer:
    """hf3fs_crc_coalescer: per-IO ChecksumInfo::create requests from many
    threads, hashed in batched device launches (include/hf3fs_crc.h)."""

    def __init__(self, device=None, **opts):
        L = load()
        o = CoalescerOptions()
        L.hf3fs_crc_coalescer_default_options(ctypes.byref(o))
        if device is not None:
            o.device = device
        for k, v in opts.items():
            setattr(o, k, v)
        h = ctypes.c_void_p()
        check(L.hf3fs_crc_coalescer_create(ctypes.byref(o), ctypes.byref(h)))
        self._h = h

    def create_one(self, ctype, buf, length, start=0xFFFFFFFF, flags=0):
        """Blocking create; `buf` is an address (int), a torch tensor or, with
        REQ_HOST_COPY, any host buffer exposing the buffer protocol."""
        out = ctypes.c_uint32()
        check(load().hf3fs_crc_coalescer_create_one(self._h, ctype, _host_or_dev(buf, flags), length, start, flags,
                                                    ctypes.byref(out)))
        return int(out.value)

    def submit(self, ctype, buf, length, fn, start=0xFFFFFFFF, flags=0):
        """Asynchronous create; fn must be a DONE_FN kept alive until it runs."""
        return check(load().hf3fs_crc_coalescer_submit(self._h, ctype, _host_or_dev(buf, flags), length, start,
                                                       flags, fn, None))

    def stats(self):
        a = (ctypes.c_uint64 * 4)()
        check(load().hf3fs_crc_coalescer_stats(self._h, a))
        return dict(requests=a[0], batches=a[1], bytes=a[2], max_batch=a[3])

    def close(self):
        if self._h:
            load().hf3fs_crc_coalescer_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _host_or_dev(buf, flags):
    if isinstance(buf, int) or buf is None:
        return buf
    if hasattr(buf, "data_ptr"):
        return buf.data_ptr()
    if hasattr(buf, "ctypes"):  # numpy array
        return buf.ctypes.data
    return ctypes.addressof(ctypes.c_char.from_buffer(buf))


def host_register(ptr, length):
    d = ctypes.c_void_p()
    check(load().hf3fs_crc_host_register(ptr, length, ctypes.byref(d)))
    return int(d.value)


def host_unregister(ptr):
    return check(load().hf3fs_crc_host_unregister(ptr))
