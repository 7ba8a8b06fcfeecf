"""Helper for tests/test_offsets_past_4gib.py (not a test module, not a conftest).

Every kernel written after the hash kernels keeps block-relative quantities in 32 bits and
absolute offsets in 64; these scenarios put byte offset 2^32 (LINE) inside the tiles where the
two meet.  Two techniques:

* first offset: one device buffer of LINE + SLACK bytes of which only the last TAIL bytes are
  written; the offsets, ranges or records handed to the entry point begin a little below LINE.
  A scenario is the TAIL-byte host image of that written part plus the absolute offsets.
* ballast: a batch that starts with thousands of records of about half a MiB each, so that the
  blobs (or kept bytes) written before the ordinary tail records total just under LINE and the
  line is crossed inside the tail.  A scenario is the sizes and the tail; the ballast bytes are
  generated on the device.

Form models: csr_scenarios.tile_model, ralle_recs_model.forms and ralle_check_model.tile_forms
are the existing ones; gather_tiles() (the CSR gather producer, k2h_ralledata.hip) and
select_tiles() (the select copy kernel) are restated here.  Nothing here calls the code under
test except the device-side runners at the end, which only launch it.
"""
import ctypes
import re
import struct
from pathlib import Path

import numpy as np

import ralle_check_model as rm
import ralle_recs_model as rr

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "k2hash_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden"

LINE = 1 << 32
SLACK = 256 << 10        # bytes of the big buffer above the line
TAIL = 512 << 10         # written bytes: the last TAIL of the LINE + SLACK buffer
BIG = LINE + SLACK
TAIL0 = BIG - TAIL       # absolute offset of the written part
GAP = 64 << 10           # the four CSR streams are base pointers GAP apart into the one buffer
CANARY = 0xA5
OUT_FILL = 0xC3
SENTINEL = 0x5A5AA5A55A5AA5A5
GUARD = 64

# k2h_ralledata.hip, restated by name (constants_match_source holds them against the source)
kGatherRecs = 64         # records per block
kGatherPool = 12288      # staged bytes: the sum of the streams' aligned 16-byte hulls


def constants_match_source():
    src = (CSRC / "k2h_ralledata.hip").read_text()
    got = {n: int(re.search(r"constexpr\s+int\s+" + n + r"\s*=\s*(\d+)\s*;", src).group(1))
           for n in ("kGatherRecs", "kGatherPool")}
    return got == {"kGatherRecs": kGatherRecs, "kGatherPool": kGatherPool}, got


def _rng(*salt):
    return np.random.default_rng([40960 + int(x) for x in salt])


def _bytes(rng, n, lo=0):
    return rng.integers(lo, 256, int(n), dtype=np.uint8).tobytes()


def image(pieces, canary=CANARY):
    """The TAIL-byte host image of the big buffer's written part: canary bytes, then each
    (absolute offset, bytes) piece; pieces must lie inside it and must not overlap."""
    tail = np.full(TAIL, canary, np.uint8)
    used = np.zeros(TAIL, bool)
    for at, data in pieces:
        a = np.frombuffer(bytes(data), np.uint8)
        assert TAIL0 <= at and at + a.size <= BIG, (at, a.size)
        assert not used[at - TAIL0:at - TAIL0 + a.size].any(), "pieces overlap"
        used[at - TAIL0:at - TAIL0 + a.size] = True
        tail[at - TAIL0:at - TAIL0 + a.size] = a
    return tail


def offsets_from(first, lens):
    off = np.empty(len(lens) + 1, np.int64)
    off[0] = first
    off[1:] = first + np.cumsum(np.asarray(lens, np.int64))
    return off


def holds_line(lo, hi):
    """[lo, hi) has bytes on both sides of the line."""
    return lo < LINE < hi


# ============================================================ the CSR gather producer's model
def gather_tiles(offs, addr_mod16=(0, 0, 0, 0)):
    """Per tile of kGatherRecs records of k2h_amd_build_ralledata: the sum of its streams' aligned
    16-byte hulls and the form it takes (staged exactly when that sum is at most kGatherPool).
    offs: four offset arrays (None = stream absent); addr_mod16: each stream's pointer & 15."""
    n = len(offs[0]) - 1
    tiles = []
    for r0 in range(0, n, kGatherRecs):
        nr = min(kGatherRecs, n - r0)
        hull = 0
        for o, a in zip(offs, addr_mod16):
            if o is None:
                continue
            b, e = int(o[r0]), int(o[r0 + nr])
            if e > b:
                hull += ((a + e + 15) & ~15) - ((a + b) & ~15)
        tiles.append(dict(r0=r0, nr=nr, hull=hull, form="staged" if hull <= kGatherPool else "group"))
    return tiles


def gather_blob_off(offs):
    """blob_off of k2h_amd_build_ralledata by its closed form: 80 i + the earlier records' bytes."""
    n = len(offs[0]) - 1
    out = 80 * np.arange(n + 1, dtype=np.int64)
    for o in offs:
        if o is not None:
            out += np.asarray(o, np.int64) - int(o[0])
    return out


# ----------------------------------------------------------- row 1: build_ralledata, inputs
CSR_N = 160              # tiles 0 and 1 whole, tile 2 partial
CSR_LINE_REC = 96        # each stream's offset LINE falls just behind this record's start: tile 1


def csr_inputs(kind):
    """Four CSR streams whose own offset LINE each lies inside tile 1 (records 64..127), which is
    staged (kind "staged") or takes the group form ("group": three 5000-byte values behind the
    line).  Returns (parts, offs): parts[s] the records' byte strings of stream s, offs[s] its
    n + 1 offsets relative to the stream's own base pointer (s * GAP into the big buffer)."""
    rng = _rng(1, kind == "group")
    lens = [rng.integers(1, 41, CSR_N), rng.integers(0, 101, CSR_N), rng.integers(0, 17, CSR_N),
            rng.integers(0, 25, CSR_N)]
    if kind == "group":
        lens[1][[100, 110, 120]] = 5000
    parts = [[_bytes(rng, x) for x in ls] for ls in lens]
    offs = [offsets_from(LINE - int(ls[:CSR_LINE_REC].sum()) - 3, ls) for ls in lens]
    return parts, offs


def csr_image(parts, offs, canary=CANARY):
    return image([(s * GAP + int(offs[s][0]), b"".join(parts[s])) for s in range(4)], canary)


# ----------------------------------------------------------- row 2: build_ralledata, output
BAL_KEY = 8              # ballast key bytes


class BuildBallast:
    """NB ballast records (an 8-byte key, a value of V bytes; NB a multiple of the tile so that
    the tail starts a tile), their blobs ending 2048 bytes below the line, then the tail:
    tile A (64 small records, staged, its blob span holds the line), tile B (group form: three
    5000-byte values as kv_big has them and three of 300 KiB, which carry the VALUE stream's own
    offset over the line), tile C (40 small records, staged, every addend of its first blob
    offset already above the line)."""
    NB = 8192 - 64
    BLOB = (LINE - 2048) // NB           # 528416
    V = BLOB - 80 - BAL_KEY

    def __init__(self):
        assert self.NB % kGatherRecs == 0 and self.NB * self.BLOB == LINE - 2048
        rng = _rng(2)
        nt = 64 + 64 + 40
        kl, vl = rng.integers(1, 41, nt), rng.integers(0, 101, nt)
        vl[[64 + 9, 64 + 30, 64 + 51]] = 5000
        vl[[64 + 5, 64 + 25, 64 + 45]] = 300 << 10
        self.tail_keys = [_bytes(rng, x) for x in kl]
        self.tail_vals = [_bytes(rng, x) for x in vl]
        self.ballast_keys = np.zeros((self.NB, BAL_KEY), np.uint8)
        self.ballast_keys[:, :4] = np.arange(self.NB, dtype="<u4").view(np.uint8).reshape(-1, 4)
        self.ballast_keys[:, 4:] = rng.integers(128, 256, (self.NB, 4), dtype=np.uint8)
        self.n = self.NB + nt
        self.koff = offsets_from(0, [BAL_KEY] * self.NB + kl.tolist())
        self.voff = offsets_from(0, [self.V] * self.NB + vl.tolist())
        self.blob_off = gather_blob_off([self.koff, self.voff, None, None])
        self.ballast_bytes = self.NB * self.BLOB
        self.total = int(self.blob_off[-1])
        self.tiles = gather_tiles([self.koff, self.voff, None, None])
        self.tile_a, self.tile_b, self.tile_c = (self.NB // kGatherRecs + j for j in range(3))


# ====================================================== rows 3 and 4: blobs from range records
def shift_import(recs, by):
    a = np.array(recs, np.uint64).reshape(-1, 4).copy()
    a[:, 0] += np.uint64(by)
    a[:, 2] += np.uint64(by)
    return a


ARCHIVE_OFFS = ("offset", "key_off", "val_off", "skey_off", "attrs_off", "exdata_off")


def shift_archive(recs, by):
    a = recs.copy()
    for name in ARCHIVE_OFFS:
        a[name] += np.uint64(by)
    return a


def line_block(segs):
    """The block of kRecRecs records whose file hull (first start .. last end of its kept
    records' segments) holds the line: (block index, hull start, hull end)."""
    hit = []
    for b in range(0, len(segs), rr.R):
        spans = [(o, o + n) for s in segs[b:b + rr.R] if s is not None for o, n in s if n]
        if spans and holds_line(min(x[0] for x in spans), max(x[1] for x in spans)):
            hit.append((b // rr.R, min(x[0] for x in spans), max(x[1] for x in spans)))
    assert len(hit) == 1, hit
    return hit[0]


class RecsInput:
    """Row 3: a small file in the big buffer, placed so that the line falls inside block 1's file
    hull, with the records that describe it there.  kind: "import" or "archive"; form: "staged"
    or "direct" (import: one 20 KiB value in block 1; archive: SET_ALL records only, whose
    104-byte headers push 64 records' hull past the pool)."""

    def __init__(self, kind, form):
        self.kind, self.form = kind, form
        if kind == "import":
            data, recs = rr.ordinary_file(160, 71) if form == "staged" else rr.big_value_file("sds", 20 * 1024)
            at = recs[rr.R + 20][0] + 3          # inside the key of record 84
            self.data, local = bytes(data), np.array(recs, np.uint64).reshape(-1, 4)
            self.start = LINE - at
            self.recs = shift_import(local, self.start)
            self.local_segs = [rr.import_segments(r, len(self.data)) for r in local]
            self.segs = [rr.import_segments(r, BIG) for r in self.recs]
            self.words = self.recs.view(np.int64).reshape(-1, 4)
        else:
            case = {c.name: c for c in rr.archive_cases()}["mixed-200" if form == "staged" else "set-all-200"]
            self.data, local = case.data, case.recs
            at = int(local[rr.R + 20]["offset"]) + 40      # inside the lengths of record 84's header
            self.start = LINE - at
            self.recs = shift_archive(local, self.start)
            self.local_segs = [rr.archive_segments(r, len(self.data)) for r in local]
            self.segs = [rr.archive_segments(r, BIG) for r in self.recs]
            self.words = np.ascontiguousarray(self.recs).view(np.int64).reshape(-1, 13)
        self.forms = rr.forms(self.segs)

    def image(self, canary=CANARY):
        return image([(self.start, self.data)], canary)


class ImportBallast:
    """Row 4: NB hand-built import records at a 512 KiB stride of a file of generated bytes --
    key = 8 bytes at i * STRIDE, value = VL bytes from 9 bytes on (it runs into the next record's
    bytes: ranges may overlap, such blocks take the direct form) -- whose blobs end 2048 bytes
    below the line; then a small TSV at TAIL_AT with its own records shifted there: block A (64
    ordinary records, staged, its blobs hold the line) and block B (one 20 KiB value: direct,
    every blob of it above the line), block C (ordinary, staged, above the line)."""
    NB = 8192 - 64
    STRIDE = 512 << 10
    BLOB = (LINE - 2048) // NB
    VL = BLOB - 80 - (BAL_KEY + 1) - 1

    def __init__(self):
        assert self.NB % rr.R == 0 and self.NB * self.BLOB == LINE - 2048
        data, recs = rr.big_value_file("sds", 20 * 1024)
        self.tail_data, self.tail_local = bytes(data), recs
        self.tail_at = (self.NB - 1) * self.STRIDE + BAL_KEY + 1 + self.VL
        self.size = self.tail_at + len(self.tail_data)
        i = np.arange(self.NB, dtype=np.uint64) * np.uint64(self.STRIDE)
        ballast = np.stack([i, np.full(self.NB, BAL_KEY, np.uint64), i + np.uint64(BAL_KEY + 1),
                            np.full(self.NB, self.VL, np.uint64)], 1)
        self.recs = np.concatenate([ballast, shift_import(recs, self.tail_at)])
        self.segs = [rr.import_segments(r, self.size) for r in self.recs]
        self.forms = rr.forms(self.segs)
        self.ballast_bytes = self.NB * self.BLOB
        sizes = np.array([80 + kl + 1 + vl + 1 for _, kl, _, vl in self.recs.tolist()], np.int64)
        self.blob_off = offsets_from(0, sizes)
        self.total = int(self.blob_off[-1])
        self.block_a = self.NB // rr.R


# ========================================================================= row 5: the check
CHECK_N = 192
CHECK_LINE_BLOB = 96


def check_stream(oracle, kind):
    """A stream of the oracle's blobs whose blob 96 (tile 1) holds the line, with one blob per
    non-OK status planted behind it in the same tile.  "staged": tile 1 is staged; "direct":
    values of 300-600 bytes (the hull passes the stage) and a 79-byte blob (BAD_SPAN, which alone
    sends its tile to the direct form).  Returns (bytes, absolute offsets, {blob: status})."""
    direct = kind == "direct"
    recs = rm.records(oracle, CHECK_N, klen=(2, 65), vlen=(300, 601) if direct else (1, 201), seed=40 + direct,
                      p_empty=0)
    buf, off = rm.stream_of(oracle, recs)
    blobs = rm.split(buf, off)
    want = {}

    def plant(i, status, fn):
        fn(blobs[i])
        want[i] = status
    plant(100, rm.BAD_HASH, lambda b: rm.put(b, 0, rm.F_HASH, rm.get(b, 0, rm.F_HASH) ^ (1 << 40)))
    plant(103, rm.BAD_SUBHASH, lambda b: rm.put(b, 0, rm.F_SUBHASH, rm.get(b, 0, rm.F_SUBHASH) ^ 1))
    plant(106, rm.NO_KEY, lambda b: rm.put(b, 0, rm.F_KLEN, 0))
    plant(109, rm.EMPTY, lambda b: [rm.put(b, 0, f, 0) for f in (rm.F_KLEN, rm.F_VLEN, rm.F_SLEN, rm.F_ALEN)])
    plant(112, rm.BAD_RANGE, lambda b: rm.put(b, 0, rm.F_KPOS, 79))
    plant(115, rm.BAD_RANGE, lambda b: rm.put(b, 0, rm.F_VPOS, len(b) + 1 - rm.get(b, 0, rm.F_VLEN)))
    if direct:
        blobs.insert(118, bytearray(b"\x01" * 79))
        want[118] = rm.BAD_SPAN
    buf, off = rm.join(blobs)
    first = LINE - off[CHECK_LINE_BLOB] - 5
    return bytes(buf), [first + x for x in off], want


CHECK_RANGE = rm.Range(1, 3, 1, 2, 5)


# ======================================================================== rows 6 and 7: select
def select_tiles(off, keep, size, out_mod16=0):
    """Per tile of SEL_TILE blobs of k2h_amd_ralledata_select: where its kept bytes go (dst0),
    how many (bytes), the pieces of 16 destination bytes they span and the form: "tabled" when
    those are at most SEL_TAB, else "searched"; "none" without kept bytes.  x[j]: the kept bytes
    of the tile before blob j (the kernel's delta[j] is off[j] - x[j])."""
    off = [int(v) for v in off]
    n = len(off) - 1
    tiles, d0 = [], 0
    for r0 in range(0, n, rm.SEL_TILE):
        nr = min(rm.SEL_TILE, n - r0)
        x, B = [], 0
        for i in range(r0, r0 + nr):
            x.append(B)
            if keep[i] and off[i] <= off[i + 1] <= size:
                B += off[i + 1] - off[i]
        a = (out_mod16 + d0) & 15
        pieces = (a + B + 15) >> 4
        tiles.append(dict(r0=r0, nr=nr, dst0=d0, bytes=B, x=x, pieces=pieces,
                          form="none" if not B else "tabled" if pieces <= rm.SEL_TAB else "searched"))
        d0 += B
    return tiles


SEL_N = 300
SEL_LINE_BLOB = 32       # early in tile 0: behind it, off[j] - x[j] has a non-zero high half


def select_input(kind):
    """300 blobs of arbitrary bytes (select does not read headers), blob 32 holding the line, a
    random half kept.  "tabled": 80-280 bytes each; "searched": 500-900, tile 0's kept bytes pass
    the piece table.  Returns (bytes, absolute offsets, keep)."""
    rng = _rng(6, kind == "searched")
    lens = rng.integers(500, 901, SEL_N) if kind == "searched" else rng.integers(80, 281, SEL_N)
    rel = offsets_from(0, lens)
    keep = (rng.random(SEL_N) < 0.5).astype(np.uint8)
    off = rel + (LINE - int(rel[SEL_LINE_BLOB]) - 7)
    return _bytes(rng, rel[-1]), off, keep


class SelectBallast:
    """Row 7: NB ballast blobs of STRIDE bytes (NB a multiple of the select tile), all kept, ending
    4096 bytes below the line; then 300 tail blobs of 80-280 bytes, a random half kept."""
    NB = 8192 - 256
    STRIDE = (LINE - 4096) // NB

    def __init__(self):
        assert self.NB % rm.SEL_TILE == 0 and self.NB * self.STRIDE == LINE - 4096
        rng = _rng(7)
        lens = rng.integers(80, 281, SEL_N)
        self.ballast_bytes = self.NB * self.STRIDE
        self.tail = _bytes(rng, lens.sum())
        self.off = offsets_from(0, [self.STRIDE] * self.NB + lens.tolist())
        self.n = self.NB + SEL_N
        self.size = int(self.off[-1])
        self.keep = np.ones(self.n, np.uint8)
        self.keep[self.NB:] = rng.random(SEL_N) < 0.5
        kept = np.flatnonzero(self.keep)
        self.index = kept.astype(np.uint64)
        self.out_off = offsets_from(0, (self.off[1:] - self.off[:-1])[kept]).astype(np.uint64)
        self.kept_bytes = int(self.out_off[-1])
        self.line_tile = self.NB // rm.SEL_TILE


# ====================================================================== row 8: the archive scan
SCOM = 104
MAGIC = b"\nK2H_"


def golden_archive():
    """(file bytes, host-scan records, the 64 records' bytes) of tests/golden/archive.k2har."""
    from k2hash_amd import archive
    f = (GOLDEN / "archive.k2har").read_bytes()
    recs = archive.scan(f)    # the host scan, pinned to archive.json by test_archive.py
    ends = [int(r["offset"]) for r in recs[1:]] + [len(f)]
    return f, recs, [f[int(r["offset"]):e] for r, e in zip(recs, ends)]


def set_all_header(command, key_len, val_len):
    """The 104-byte header of a SCOM_SET_ALL record with a key and a value (include/k2hash_amd.h
    section 5): szCommand, type 0, the five lengths, the five positions from the record's start
    (subkeys and attrs empty behind the value; exdata, which the type does not carry, at 104)."""
    end = SCOM + key_len + val_len
    head = command + struct.pack("<q", 0) + struct.pack("<5Q", key_len, val_len, 0, 0, 0) + \
        struct.pack("<5Q", SCOM, SCOM + key_len, end, end, SCOM)
    assert len(head) == SCOM
    return head


def set_all_rec(key_len, val_len):
    """That record at offset 0 as the scan must report it (archive.REC_DTYPE), built by hand."""
    from k2hash_amd import archive
    r = np.zeros(1, archive.REC_DTYPE)
    end = SCOM + key_len + val_len
    r["key_off"], r["key_len"], r["val_off"], r["val_len"] = SCOM, key_len, SCOM + key_len, val_len
    r["skey_off"], r["attrs_off"], r["exdata_off"] = end, end, SCOM
    return r


HEAD_KEY = b"the-one-giant-record"
SCAN_TAIL_N = 200
SCAN_LINE_REC = 100
SCAN_CASES = ("header", "prefix-1", "prefix-2", "prefix-3", "prefix-4", "key", "record-at-line", "decoys")


class ScanFile:
    """One SET_ALL record whose value is a run of zero bytes, then a tail of 200 records drawn
    from the golden file's 64 (for "decoys": every fourth a SET_ALL record whose value holds two
    "\\nK2H_" prefixes), placed so that tail record 100
      header:          has byte 40 of its header on the line (the lengths at [24, 64) straddle it)
      prefix-k:        starts k bytes below the line
      key:             has the line inside its key
      record-at-line:  starts exactly on it
      decoys:          as key."""

    def __init__(self, case):
        f, recs, parts = golden_archive()
        from k2hash_amd import archive
        self.command = f[int(recs[0]["offset"]):int(recs[0]["offset"]) + 16]
        assert int(recs[0]["type"]) == 0 and self.command.startswith(MAGIC)
        rng = _rng(8, SCAN_CASES.index(case))
        body = [parts[i] for i in rng.integers(0, 64, SCAN_TAIL_N)]
        if case == "decoys":
            for j in range(1, SCAN_TAIL_N, 4):
                key, val = b"decoy%d" % j, b"xx" + MAGIC + b"y" * (j % 7) + MAGIC + b"zz"
                body[j] = set_all_header(self.command, len(key), len(val)) + key + val
        self.tail = b"".join(body)
        self.tail_recs = archive.scan(self.tail)
        assert self.tail_recs.size == SCAN_TAIL_N and not self.tail_recs["status"].any()
        r = self.tail_recs[SCAN_LINE_REC]
        if case == "header":
            at = int(r["offset"]) + 40
        elif case.startswith("prefix-"):
            at = int(r["offset"]) + int(case[-1])
        elif case == "record-at-line":
            at = int(r["offset"])
        else:
            assert int(r["key_len"]) >= 2
            at = int(r["key_off"]) + int(r["key_len"]) // 2
        self.case = case
        self.tail_at = LINE - at
        self.val_len = self.tail_at - SCOM - len(HEAD_KEY)
        self.head = set_all_header(self.command, len(HEAD_KEY), self.val_len) + HEAD_KEY
        self.size = self.tail_at + len(self.tail)
        self.want = np.concatenate([set_all_rec(len(HEAD_KEY), self.val_len),
                                    shift_archive(self.tail_recs, self.tail_at)])

    def line_rec(self):
        return self.want[1 + SCAN_LINE_REC]


# ===================================================================== row 9: the hash-only calls
RANGE_LENS = (1, 16, 17, 150)


def line_ranges():
    """(starts, lens): keys of 1, 16, 17 and 150 bytes (pads 15, 0, 15, 10) that end on the last
    byte below the line, begin on it, and hold it; and a key of 16 whose first chunk is the 16
    bytes below the line (pad 0, one chunk on either side)."""
    s, n = [], []
    for L in RANGE_LENS:
        s += [LINE - L, LINE] + ([LINE - L // 2, LINE - 1, LINE - L + 1] if L > 1 else [])
        n += [L] * (5 if L > 1 else 2)
    s.append(LINE - 16)
    n.append(32)
    return np.array(s, np.int64), np.array(n, np.int64)


def near_start_ranges():
    """key_off 0..15 x key lengths 1..32 over a file of 64 + bytes: every pad p = 16 k - len at
    every offset below 16, so off < p (hash_raw_checked's chunk0_from_bytes arm), off == p and
    off > p all occur."""
    s = np.repeat(np.arange(16), 32)
    n = np.tile(np.arange(1, 33), 16)
    return s.astype(np.int64), n.astype(np.int64)


# ================================================================================ device side
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    from k2hash_amd.batch import _stream_handle
    return _stream_handle(None)


def big_buffer(cuda):
    """The LINE + SLACK buffer, unwritten (torch.empty)."""
    import torch
    big = torch.empty(BIG, dtype=torch.uint8, device=cuda)
    assert big.data_ptr() % 128 == 0
    return big


def load_tail(big, tail):
    import torch
    assert tail.size == TAIL
    big[TAIL0:] = torch.from_numpy(tail).to(big.device)


def guarded(torch, cuda, nbytes, shift=0, fill=OUT_FILL):
    """(whole, view): a byte buffer of nbytes that starts GUARD + shift bytes into a filled
    allocation with GUARD filled bytes behind it."""
    whole = torch.full((GUARD + shift + nbytes + GUARD,), fill, dtype=torch.uint8, device=cuda)
    assert whole.data_ptr() % 128 == 0 and GUARD % 16 == 0
    return whole, whole[GUARD + shift:GUARD + shift + nbytes]


def guards_intact(torch, whole, view, fill=OUT_FILL):
    lo = view.data_ptr() - whole.data_ptr()
    return bool((whole[:lo] == fill).all()) and bool((whole[lo + view.numel():] == fill).all())


def rows_equal(torch, a, b, rows=1024):
    """torch.equal of two (n, m) device views, `rows` rows at a time: the comparison's
    intermediate stays a fraction of the operands (the views may be strided)."""
    assert a.shape == b.shape and a.dim() == 2
    return all(torch.equal(a[r:r + rows], b[r:r + rows]) for r in range(0, a.shape[0], rows))


def sentinel_words(torch, cuda, n):
    full = torch.full((n + GUARD,), SENTINEL, dtype=torch.int64, device=cuda)
    return full, full[:n]


def words_back(torch, full, n, what):
    a = full.cpu().numpy().view(np.uint64)
    assert (a[n:] == np.uint64(SENTINEL)).all(), f"{what}: written past entry {n}"
    return a[:n]


def run_build(cuda, ptrs, offs, n, out, total):
    """k2h_amd_build_ralledata over streams given as (bytes tensor or None, offsets array or
    None) pairs, into `out` (a guarded view); returns blob_off as a host uint64 array."""
    import torch

    from k2hash_amd import ralledata
    args = []
    for t, o in zip(ptrs, offs):
        args += [None, None] if o is None else [t, torch.from_numpy(np.ascontiguousarray(o, np.int64)).to(cuda)]
    full, boff = sentinel_words(torch, cuda, n + 1)
    ralledata.build_ralledata(*args, out=out, total=total, blob_off=boff)
    torch.cuda.synchronize()
    return words_back(torch, full, n + 1, "blob_off")


def run_check(cuda, blobs, size, off, rng, std_fnv=False):
    """k2h_amd_ralledata_check into sentinel-filled outputs: (status, route, h1, h2) on the host."""
    import torch

    from k2hash_amd import _native
    n = len(off) - 1
    d_off = torch.tensor([int(x) for x in off], dtype=torch.int64, device=cuda)
    sw, status = guarded(torch, cuda, n, fill=0xEE)
    rw, route = guarded(torch, cuda, n, fill=0xEE)
    f1, h1 = sentinel_words(torch, cuda, n)
    f2, h2 = sentinel_words(torch, cuda, n)
    r = rng.ctypes()
    _native.check(_native.batch_lib().k2h_amd_ralledata_check(
        _p(blobs), size, _p(d_off), n, ctypes.byref(r), _native.K2H_AMD_FLAG_STD_FNV if std_fnv else 0, _p(status),
        _p(route), _p(h1), _p(h2), _stream()))
    torch.cuda.synchronize()
    assert guards_intact(torch, sw, status, 0xEE) and guards_intact(torch, rw, route, 0xEE)
    return status.cpu().numpy(), route.cpu().numpy(), words_back(torch, f1, n, "h1"), words_back(torch, f2, n, "h2")


def run_select(cuda, blobs, size, off, keep, out, want_kept_bytes):
    """k2h_amd_ralledata_select into `out` (a guarded view of exactly the expected bytes) and
    sentinel-filled out_off / index: (kept, kept_bytes, out_off, index) with host arrays."""
    import torch

    from k2hash_amd import _native
    n = len(off) - 1
    d_off = torch.from_numpy(np.ascontiguousarray(off, np.int64)).to(cuda)
    d_keep = torch.from_numpy(np.ascontiguousarray(keep, np.uint8)).to(cuda)
    fo, ooff = sentinel_words(torch, cuda, n + 1)
    fi, index = sentinel_words(torch, cuda, n)
    kept, kb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert out.numel() == want_kept_bytes
    _native.check(_native.batch_lib().k2h_amd_ralledata_select(
        _p(blobs), size, _p(d_off), n, _p(d_keep), _p(out), out.numel(), _p(ooff), _p(index), ctypes.byref(kept),
        ctypes.byref(kb), _stream()))
    torch.cuda.synchronize()
    k = int(kept.value)
    a = fo.cpu().numpy().view(np.uint64)
    assert (a[k + 1:] == np.uint64(SENTINEL)).all(), "out_off written past entry kept"
    b = fi.cpu().numpy().view(np.uint64)
    assert (b[k:] == np.uint64(SENTINEL)).all(), "index written past entry kept - 1"
    return k, int(kb.value), a[:k + 1], b[:k]


def run_scan_prehash(cuda, file, size, cap):
    """k2h_amd_archive_scan_prehash_device with room for exactly cap records: (count, records as
    a REC_DTYPE array, h1, h2); rows and hashes past cap must keep their sentinel."""
    import torch

    from k2hash_amd import _native, archive
    fr, recs = sentinel_words(torch, cuda, cap * archive.REC_WORDS)
    f1, h1 = sentinel_words(torch, cuda, cap)
    f2, h2 = sentinel_words(torch, cuda, cap)
    cnt = ctypes.c_uint64(0)
    _native.check(_native.batch_lib().k2h_amd_archive_scan_prehash_device(
        _p(file), size, _p(recs), cap, ctypes.byref(cnt), _p(h1), _p(h2), None, None, 0, _stream()))
    torch.cuda.synchronize()
    n = int(cnt.value)
    rows = words_back(torch, fr, cap * archive.REC_WORDS, "recs")
    return n, rows[:n * archive.REC_WORDS].copy().view(archive.REC_DTYPE).reshape(-1), \
        words_back(torch, f1, cap, "h1")[:n], words_back(torch, f2, cap, "h2")[:n]
