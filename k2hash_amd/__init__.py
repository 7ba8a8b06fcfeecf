"""k2hash_amd -- MI355X-native key-hash path for yahoojapan/k2hash.

Scope: the default FNV-1a key hash of lib/k2hashfunc.cc,
as (1) a bit-exact drop-in hash plugin (C ABI, include/k2hash_amd.h section 1)
and (2) a batch C ABI backed by hand-written gfx950 HIP kernels (section 2).

  hashfunc   mirror of the reference interface: k2h_hash, k2h_second_hash,
             k2h_hash_version, K2HashDynLib, K2H_HASH_FUNC ...
  batch      device/host batch hashing, the fused bucket-index epilogue
             (K2HShm::GetKIndexPos / GetCKIndex positions), synthetic workloads
  ralledata  RALLEDATA direct-set blobs: built on the GPU (from CSR streams, or straight
             from the records of a scanned import file or archive), and blob streams
             checked, routed by hash range, compacted and split into owner or lock
             partitions there, written out as a k2hash archive, and two streams joined by
             identity (what an incoming stream changes in a held one)
  subkeys    the subkeys segments of a blob stream read there: names as edges between blobs,
             the subtree a set of roots reaches, and the stream with it kept or removed
  unlink     subkey names taken out of the lists that carry them: the first calls that rewrite
             blobs (drop_mask, unlink_subkeys, prune_ralledata; also reachable through subkeys)
  archive    k2hash archives scanned and prehashed on the GPU, and transaction logs folded to
             the records that still matter under Load's rule (fold_device, compact_device)
  apply      a transaction log applied to a held blob stream: replication, and log -> snapshot
             (apply_log, apply_records)
  barrier    the OW_VAL and RENAME records an apply stops at, executed on the held stream in
             place, and a whole log replayed with them (execute_barrier, replay_log)
  delta      the inverse: from a held and a new blob stream to the transaction log that turns
             the one into the other (delta_log, delta_records)
  find       keys looked up in a held blob stream: the stream indexed once, a batch of keys found
             through the index (Get without a table), and one segment of a list of blobs fetched
             as a CSR column (index_stream, find_keys, fetch_segments, get_values)
  shard      multi-GPU partitioning and the RCCL gather of hashes
"""
from .hashfunc import (K2H_2ND_HASH_FUNC, K2H_HASH_FUNC, K2H_HASH_VER_FUNC, K2HashDynLib, k2h_hash,
                       k2h_hash_version, k2h_second_hash)
from .batch import (bucket_index, hash_csr, hash_csr_host, hash_csr_index, hash_fixed, hash_fixed_host,
                    hash_fixed_index, synth_bytes, synth_offsets, unpack_kindex, version)
from .apply import Applied, apply_log, apply_records
from .archive import compact_device, fold_device
from .barrier import Executed, Replayed, execute_barrier, replay_log
from .delta import Delta, delta_log, delta_records
from .find import Found, StreamIndex, fetch_segments, find_keys, get_values, index_stream
from .ralledata import (Diff, HashRange, Times, TimeWindow, archive_to_ralledata, blob_times, check_ralledata,
                        dedup_ralledata, diff_ralledata, import_file_to_archive, import_file_to_ralledata, import_to_ralledata, make_hash_range, partition_ralledata,
                        ralledata_to_archive, route_ralledata, select_ralledata)
from .subkeys import (Reach, SubkeyEdges, Unlinked, drop_mask, prune_ralledata, reach_subkeys, subkey_edges,
                      subtree_ralledata, unlink_subkeys)

__all__ = [
    "k2h_hash", "k2h_second_hash", "k2h_hash_version", "K2HashDynLib", "K2H_HASH_FUNC",
    "K2H_2ND_HASH_FUNC", "K2H_HASH_VER_FUNC", "hash_fixed", "hash_csr", "hash_fixed_host",
    "hash_csr_host", "synth_bytes", "synth_offsets", "version", "bucket_index", "hash_fixed_index",
    "hash_csr_index", "unpack_kindex", "check_ralledata", "select_ralledata", "route_ralledata", "HashRange",
    "make_hash_range", "import_to_ralledata", "archive_to_ralledata", "import_file_to_ralledata",
    "dedup_ralledata", "partition_ralledata", "ralledata_to_archive", "import_file_to_archive",
    "blob_times", "TimeWindow", "Times", "fold_device", "compact_device", "diff_ralledata", "Diff",
    "subkey_edges", "reach_subkeys", "subtree_ralledata", "SubkeyEdges", "Reach",
    "drop_mask", "unlink_subkeys", "prune_ralledata", "Unlinked", "apply_log", "apply_records", "Applied",
    "delta_log", "delta_records", "Delta", "execute_barrier", "replay_log", "Executed", "Replayed",
    "index_stream", "find_keys", "fetch_segments", "get_values", "StreamIndex", "Found",
]
