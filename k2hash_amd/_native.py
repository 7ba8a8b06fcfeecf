"""ctypes binding of the k2hash_amd C ABI (include/k2hash_amd.h).

The native libraries are built in-tree by ``k2hash_amd/csrc/Makefile`` into
``k2hash_amd/lib/``.  There is no Python fallback for the hash path: if the
library is missing this module raises, loudly, on first use.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

LIB_DIR = Path(__file__).resolve().parent / "lib"
BATCH_LIB = LIB_DIR / "libk2hash_amd.so"
PLUGIN_LIB = LIB_DIR / "libk2hfnv_plugin.so"

K2H_AMD_OK = 0
K2H_AMD_EINVAL = -1
K2H_AMD_EHIP = -2
K2H_AMD_ENOMEM = -3
K2H_AMD_ENODEV = -4
K2H_AMD_FLAG_STD_FNV = 0x1
K2H_AMD_FLAG_CSTR = 0x2
K2H_AMD_IMPORT_TSV, K2H_AMD_IMPORT_MDBM = 0, 1
K2H_AMD_SCOM_HEADER = 104

_u64 = ctypes.c_uint64
_p = ctypes.c_void_p


class Table(ctypes.Structure):
    """k2h_amd_table (include/k2hash_amd.h section 3)."""
    _fields_ = [("cur_mask", ctypes.c_uint64), ("collision_mask", ctypes.c_uint64), ("assigned", ctypes.c_void_p)]


_tp = ctypes.POINTER(Table)


class HashRange(ctypes.Structure):
    """k2h_amd_hash_range (include/k2hash_amd.h section 4b): the arguments of
    K2HShm::GetElementListToBinary's selection (lib/k2hshmdirect.cc:103, 118-131)."""
    _fields_ = [("target_hash", ctypes.c_uint64), ("target_max_hash", ctypes.c_uint64),
                ("target_hash_range", ctypes.c_int64), ("old_hash", ctypes.c_uint64),
                ("old_max_hash", ctypes.c_uint64)]


_rp = ctypes.POINTER(HashRange)

K2H_AMD_PART_MAX = 256
K2H_AMD_PART_NONE = 0xFFFFFFFF
K2H_AMD_PART_IDS, K2H_AMD_PART_OWNER, K2H_AMD_PART_MASK = 0, 1, 2


class PartRule(ctypes.Structure):
    """k2h_amd_part_rule (include/k2hash_amd.h section 4b'')."""
    _fields_ = [("kind", ctypes.c_uint32), ("parts", ctypes.c_uint32), ("max_hash", ctypes.c_uint64),
                ("span", ctypes.c_uint64), ("mask", ctypes.c_uint64)]


_prp = ctypes.POINTER(PartRule)
_u64p = ctypes.POINTER(ctypes.c_uint64)

K2H_AMD_WIN_START, K2H_AMD_WIN_END, K2H_AMD_WIN_EXPIRE = 1, 2, 4
K2H_AMD_TIMES_MTIME, K2H_AMD_TIMES_EXPIRE, K2H_AMD_TIMES_CUT, K2H_AMD_TIMES_ATTRS = 1, 2, 4, 8


class Timespec(ctypes.Structure):
    """k2h_amd_timespec (include/k2hash_amd.h section 4b'''')."""
    _fields_ = [("sec", ctypes.c_int64), ("nsec", ctypes.c_int64)]


class TimeWindowStruct(ctypes.Structure):
    """k2h_amd_time_window (include/k2hash_amd.h section 4b'''')."""
    _fields_ = [("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("start", Timespec), ("end", Timespec),
                ("now", Timespec)]


class DiffTimes(ctypes.Structure):
    """k2h_amd_diff_times (include/k2hash_amd.h section 4b'''''): the pts the feed will use and the clock."""
    _fields_ = [("pts", Timespec), ("now", Timespec)]


K2H_AMD_DIFF_PART, K2H_AMD_DIFF_FOUND, K2H_AMD_DIFF_VAL, K2H_AMD_DIFF_SKEY = 0x01, 0x02, 0x04, 0x08
K2H_AMD_DIFF_ATTRS, K2H_AMD_DIFF_DATA, K2H_AMD_DIFF_REPEAT, K2H_AMD_DIFF_APPLY = 0x10, 0x20, 0x40, 0x80

K2H_AMD_SKEY_PART, K2H_AMD_SKEY_HAS, K2H_AMD_SKEY_BAD = 0x1, 0x2, 0x4
K2H_AMD_UNLINK_REWRITTEN, K2H_AMD_UNLINK_EMPTIED, K2H_AMD_UNLINK_KEY_ONLY = 0x1, 0x2, 0x4
K2H_AMD_APPLY_TOUCHED, K2H_AMD_APPLY_SUPERSEDED, K2H_AMD_APPLY_LEFT_OUT = 1, 2, 3
K2H_AMD_BARRIER_EXECUTED, K2H_AMD_BARRIER_NOT_FOUND, K2H_AMD_BARRIER_NEW_EXISTS = 0, 1, 2
K2H_AMD_BARRIER_BAD_RECORD, K2H_AMD_BARRIER_NOT_A_BARRIER = 3, 4
K2H_AMD_BARRIER_CREATED, K2H_AMD_BARRIER_GAP = 1, 2
K2H_AMD_BARRIER_COUNT_ONLY, K2H_AMD_BARRIER_MAX_RUN = 0x100, 256
K2H_AMD_DELTA_SET_ALL, K2H_AMD_DELTA_REPLACE_VAL, K2H_AMD_DELTA_REPLACE_SKEY = 0x01, 0x02, 0x04
K2H_AMD_DELTA_REPLACE_ATTRS, K2H_AMD_DELTA_DEL_KEY = 0x08, 0x10
K2H_AMD_FIND_PART, K2H_AMD_FIND_FOUND, K2H_AMD_FIND_ATTRS, K2H_AMD_FIND_EXPIRED = 0x01, 0x02, 0x04, 0x08
K2H_AMD_FIND_BAD_INDEX = 0x80
K2H_AMD_SEG_KEY, K2H_AMD_SEG_VAL, K2H_AMD_SEG_SKEY, K2H_AMD_SEG_ATTRS = 0, 1, 2, 3

_twp = ctypes.POINTER(TimeWindowStruct)
_dtp = ctypes.POINTER(DiffTimes)
_tsp = ctypes.POINTER(Timespec)

# name -> (restype, argtypes); mirrors include/k2hash_amd.h
SIGNATURES = {
    "k2h_hash": (_u64, [_p, ctypes.c_size_t]),
    "k2h_second_hash": (_u64, [_p, ctypes.c_size_t]),
    "k2h_hash_version": (ctypes.c_char_p, []),
    "k2h_amd_hash_fixed": (ctypes.c_int, [_p, _u64, _u64, _p, _p, ctypes.c_uint32, _p]),
    "k2h_amd_hash_csr": (ctypes.c_int, [_p, _p, _u64, _p, _p, ctypes.c_uint32, _p]),
    "k2h_amd_hash_fixed_host": (ctypes.c_int, [_p, _u64, _u64, _p, _p, ctypes.c_uint32, ctypes.c_int]),
    "k2h_amd_hash_csr_host": (ctypes.c_int, [_p, _p, _u64, _p, _p, ctypes.c_uint32, ctypes.c_int]),
    "k2h_amd_bucket_index": (ctypes.c_int, [_p, _u64, _u64, _u64, _p, _p, _p]),
    "k2h_amd_hash_fixed_index": (ctypes.c_int, [_p, _u64, _u64, _p, _p, ctypes.c_uint32, _u64, _u64, _p, _p, _p]),
    "k2h_amd_hash_csr_index": (ctypes.c_int, [_p, _p, _u64, _p, _p, ctypes.c_uint32, _u64, _u64, _p, _p, _p]),
    "k2h_amd_bucket_index_table": (ctypes.c_int, [_p, _u64, _tp, _p, _p, _p, _p]),
    "k2h_amd_hash_fixed_index_table": (ctypes.c_int, [_p, _u64, _u64, _p, _p, ctypes.c_uint32, _tp, _p, _p, _p, _p]),
    "k2h_amd_hash_csr_index_table": (ctypes.c_int, [_p, _p, _u64, _p, _p, ctypes.c_uint32, _tp, _p, _p, _p, _p]),
    "k2h_amd_ralledata_size": (_u64, [_u64, _u64, _u64, _u64, _u64]),
    "k2h_amd_build_ralledata": (ctypes.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _u64, _p, _p, ctypes.c_uint32, _p]),
    "k2h_amd_build_ralledata_host": (ctypes.c_int,
                                     [_p, _p, _p, _p, _p, _p, _p, _p, _u64, _p, _p, ctypes.c_uint32, ctypes.c_int]),
    "k2h_amd_ralledata_check": (ctypes.c_int, [_p, _u64, _p, _u64, _rp, ctypes.c_uint32, _p, _p, _p, _p, _p]),
    "k2h_amd_ralledata_select": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, _u64, _p, _p, _u64p, _u64p, _p]),
    "k2h_amd_ralledata_dedup": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, _p, _u64p, _p]),
    "k2h_amd_ralledata_times": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _twp, _p, _p, _p, _p, _p, _p]),
    "k2h_amd_ralledata_dedup_mtime": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, _p, _u64p, _tsp, _p]),
    "k2h_amd_ralledata_diff": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, _u64, _p, _u64, _p, _dtp, _p, _p, _p, _u64p,
                                              _p]),
    "k2h_amd_ralledata_subkeys": (ctypes.c_int, [_p, _u64, _p, _u64, _p, ctypes.c_uint32, _p, _p, _p, _p, _u64, _u64p,
                                                 _p]),
    "k2h_amd_ralledata_reach": (ctypes.c_int, [_p, _p, _p, _u64, _p, _u64, _p, _u64p, _p]),
    "k2h_amd_ralledata_unlink": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, _p, _p, _p, _u64, _p, _p, _p, _u64p, _p]),
    "k2h_amd_subkeys_drop_mask": (ctypes.c_int, [_p, _u64, _p, _u64, ctypes.c_int, _p, _p]),
    "k2h_amd_ralledata_partition": (ctypes.c_int, [_p, _u64, _p, _u64, _prp, _p, _p, _p, _u64, _p, _p, _p, _u64p,
                                                   _u64p, _p]),
    "k2h_amd_import_ralledata": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _u64, _p, _u64p, ctypes.c_uint32, _p]),
    "k2h_amd_archive_ralledata": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _u64, _p, _u64p, ctypes.c_uint32, _p]),
    "k2h_amd_ralledata_archive": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, _u64, _p, _u64p, _u64p, _p]),
    "k2h_amd_ralledata_delta": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, _u64, _p, _u64, _p, _p, _p, _u64, _p, _p,
                                               _u64p, _p]),
    "k2h_amd_ralledata_index_size": (_u64, [_u64]),
    "k2h_amd_ralledata_index": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, _u64, _u64p, _p]),
    "k2h_amd_ralledata_find": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, _u64, _p, _u64, _p, _p, ctypes.c_uint32, _tsp,
                                              _p, _p, _p, _u64p, _p]),
    "k2h_amd_ralledata_fetch": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _u64, _p, ctypes.c_uint32, _p, _u64, _p, _p,
                                               _u64p, _p]),
    "k2h_amd_hash_ranges": (ctypes.c_int, [_p, _p, _p, _u64, _p, _p, ctypes.c_uint32, _p]),
    "k2h_amd_archive_scan": (ctypes.c_int, [_p, _u64, _p, _u64, _p]),
    "k2h_amd_archive_prehash_host": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, _p, _p, ctypes.c_uint32, ctypes.c_int]),
    "k2h_amd_archive_scan_device": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p]),
    "k2h_amd_archive_prehash": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, _p, _p, ctypes.c_uint32, _p]),
    "k2h_amd_archive_scan_prehash_device": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, _p, _p, _p,
                                                           ctypes.c_uint32, _p]),
    "k2h_amd_archive_fold": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, _p, _u64p, _p]),
    "k2h_amd_archive_apply": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, _u64, _p, _u64, _p, _p, _p, ctypes.c_uint32,
                                             _p, _u64, _p, _p, _p, _u64p, _u64p, _p]),
    "k2h_amd_archive_barrier": (ctypes.c_int, [_p, _u64, _u64, _p, _u64, _p, _p, _u64, _p, _u64, _u64, _p, _p, _p, _p, _p,
                                               ctypes.c_uint32, _u64p, _p]),
    "k2h_amd_import_scan": (ctypes.c_int, [_p, _u64, ctypes.c_int, _p, _u64, _p]),
    "k2h_amd_import_prehash_host": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, ctypes.c_uint32, ctypes.c_int]),
    "k2h_amd_import_scan_device": (ctypes.c_int, [_p, _u64, ctypes.c_int, _p, _u64, _p, _p]),
    "k2h_amd_import_prehash": (ctypes.c_int, [_p, _u64, _p, _u64, _p, _p, ctypes.c_uint32, _p]),
    "k2h_amd_import_scan_prehash_device": (ctypes.c_int, [_p, _u64, ctypes.c_int, _p, _u64, _p, _p, _p,
                                                          ctypes.c_uint32, _p]),
    "k2h_amd_version": (ctypes.c_char_p, []),
    "k2h_amd_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "k2h_amd_synth_bytes": (ctypes.c_int, [_p, _u64, _u64, _u64, _p]),
    "k2h_amd_synth_lengths": (ctypes.c_int, [_p, _u64, _u64, _u64, ctypes.c_uint32, ctypes.c_uint32, _p]),
}

PLUGIN_SYMBOLS = ("k2h_hash", "k2h_second_hash", "k2h_hash_version")

_batch = None


class NativeError(RuntimeError):
    """A k2hash_amd C-ABI call returned a negative K2H_AMD_E* code."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"k2hash_amd error {code}: {msg}")
        self.code = code


def _bind(lib: ctypes.CDLL, names) -> ctypes.CDLL:
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = SIGNATURES[name]
    return lib


def batch_lib() -> ctypes.CDLL:
    """The batch library (HIP kernels + plugin symbols).  Raises if not built."""
    global _batch
    if _batch is None:
        # One HIP runtime per process: torch ships its own libamdhip64 (soname
        # libamdhip64.so.7, like /opt/rocm's).  Loading torch first lets this library's
        # libamdhip64.so.7 dependency bind to that copy; the other order leaves two
        # runtimes in the process and torch then sees no GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        path = BATCH_LIB
        if not path.exists():
            raise RuntimeError(
                f"k2hash_amd native library missing: {path} "
                "(build it with `make -C k2hash_amd/csrc` or __graft_entry__.build())")
        _batch = _bind(ctypes.CDLL(str(path)), SIGNATURES.keys())
    return _batch


def plugin_lib(path: str | os.PathLike | None = None) -> ctypes.CDLL:
    """A library exposing only the three plugin symbols (default: libk2hfnv_plugin.so)."""
    p = Path(path) if path else PLUGIN_LIB
    if not p.exists():
        raise RuntimeError(f"k2hash_amd plugin library missing: {p}")
    return _bind(ctypes.CDLL(str(p)), PLUGIN_SYMBOLS)


def check(rc: int) -> None:
    if rc != K2H_AMD_OK:
        msg = batch_lib().k2h_amd_strerror(rc).decode(errors="replace")
        raise NativeError(rc, msg)
