"""3fs_amd -- MI355X-native batched chunk-integrity engine for 3FS's ChecksumInfo path.

Import with importlib (the directory name starts with a digit):
    hf = importlib.import_module("3fs_amd")

Contents:
  csrc/           HIP kernels (gfx950) + the C ABI (include/hf3fs_crc.h)
  lib/            built libhf3fs_crc.so (python 3fs_amd/build.py)
  _lib.py         ctypes binding of the C ABI
  checksum.py     ChecksumInfo mirror (Common.h:113-202)
  node.py         multi-GPU sharding by chain id + RCCL digest all-gather
"""
from . import _lib  # noqa: F401
from ._lib import (CHECKSUM_MISMATCH, CRC32, CRC32C, DEVICE_ERROR, FLAG_ENGINE, FLAG_SYNCING,  # noqa: F401
                   INVALID_ARG, MODE_DELTA, MODE_REFERENCE, NONE, NOT_APPLIED, OK, UPDATE_EXTEND,
                   UPDATE_TRUNCATE, UPDATE_WRITE, Hf3fsCrcError, UpdateIO, load, update_cow,
                   update_cow_scratch_bytes, update_ordered, update_ordered_scratch_bytes)
from ._lib import (SYNC_CHAIN_VER_LOW, SYNC_CHAIN_WRITING, SYNC_CHAIN_WRITING_CHECKSUM,  # noqa: F401
                   SYNC_CHECKSUM_MISMATCH, SYNC_COMMIT_VER_MISMATCH, SYNC_DUPLICATE, SYNC_EQUAL,
                   SYNC_FULL_SYNC_HEAVY, SYNC_HEAVY, SYNC_INFO_NAMES, SYNC_INFO_WORDS, SYNC_LOCAL_RECYCLING,
                   SYNC_LOCAL_UNCOMMITTED, SYNC_MATCHED, SYNC_NONE, SYNC_REMOTE_CHAIN_VER_HIGH, SYNC_REMOTE_MISS,
                   SYNC_REMOTE_ONLY, SYNC_REMOTE_UNCOMMITTED, SyncMeta, sync_plan, sync_plan_scratch_bytes,
                   sync_scrub_fill)
from ._lib import (UPDATE_COMMIT, VER_INFO_NAMES, VER_INFO_WORDS, update_ver_dtype, update_versioned,  # noqa: F401
                   update_versioned_scratch_bytes)
from ._lib import (ENGINE_INFO_NAMES, ENGINE_INFO_WORDS, engine_job_dtype, update_engine,  # noqa: F401
                   update_engine_scratch_bytes)
from ._lib import (MD5_FINAL, MD5_INIT, md5_batch, md5_hex, md5_scratch_bytes, md5_seg_dtype,  # noqa: F401
                   md5_state_dtype)
from ._lib import (CHUNK_NOT_FOUND, CLIENT_NOT_INITIALIZED, CLIENT_READ_INFO_NAMES,  # noqa: F401
                   CLIENT_READ_INFO_WORDS, CLIENT_READ_NONE, CLIENT_READ_VERIFY, ClientReadIO, ClientReadResult,
                   block_digest_dtype, client_read_batch, client_read_io_dtype, client_read_result_dtype,
                   client_read_scratch_bytes)
from ._lib import (CLIENT_INVALID_ARG, CLIENT_WRITE_DONE_NAMES, CLIENT_WRITE_DONE_WORDS,  # noqa: F401
                   CLIENT_WRITE_FROM_UPDATES, CLIENT_WRITE_INFO_NAMES, CLIENT_WRITE_INFO_WORDS, CLIENT_WRITE_NONE,
                   CLIENT_WRITE_VERIFY, INVALID_FORMAT, ClientWriteFile, ClientWriteIO, client_write_complete,
                   client_write_file_dtype, client_write_io_dtype, client_write_prepare, client_write_scratch_bytes,
                   update_io_dtype)
from ._lib import (FORWARD_COMMIT, FORWARD_DONE_NAMES, FORWARD_INFO_NAMES, FORWARD_INFO_WORDS,  # noqa: F401
                   FORWARD_NO_SUCCESSOR, FORWARD_OUT_COMMIT_CHAIN_VER, FORWARD_OUT_INLINE, FORWARD_OUT_SYNCING,
                   FORWARD_REQ_INLINE, FORWARD_REQ_SYNCING, FORWARD_RETURN, FORWARD_SEND, NO_SUCCESSOR_TARGET,
                   UPDATE_REMOVE, ForwardJob, forward_complete, forward_job_dtype, forward_prepare,
                   forward_scratch_bytes)
from ._lib import (CHUNK_METADATA_GET_ERROR, CHUNK_METADATA_NOT_FOUND, CHUNK_NOT_COMMIT,  # noqa: F401
                   CHUNK_READ_FAILED, RDMA_NO_BUF, SERVER_READ_BUF_BIG, SERVER_READ_BUF_NONE, SERVER_READ_BUF_SMALL,
                   SERVER_READ_DONE_NAMES, SERVER_READ_INFO_NAMES, SERVER_READ_INFO_WORDS, SERVER_READ_NONE,
                   SERVER_READ_XMIT_INLINE, SERVER_READ_XMIT_NONE, SERVER_READ_XMIT_RDMA, TARGET_STATE_INVALID,
                   ServerReadJob, ServerReadReq, ServerReadWr, server_read_complete, server_read_job_dtype,
                   server_read_prepare, server_read_req_dtype, server_read_scratch_bytes, server_read_wr_dtype)
from ._lib import (DATA_CORRUPTION, FILE_LEN_DYN, FILE_LEN_INFO_NAMES, FILE_LEN_INFO_WORDS,  # noqa: F401
                   FILE_LEN_MAX_OPS, META_BUSY, RANGE_INFO_NAMES, RANGE_INFO_WORDS, RANGE_MAX_COUNT, RANGE_NONE,
                   RANGE_QUERY, RANGE_REMOVE, FileLen, RangeOp, file_len_dtype, file_length, range_op_dtype,
                   range_query, range_query_scratch_bytes, sync_meta_dtype)
from .checksum import ChecksumInfo, ChecksumType  # noqa: F401
