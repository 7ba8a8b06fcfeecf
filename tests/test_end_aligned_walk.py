"""The end-aligned key walk (k2h_endwalk.h), its edge cases in one place, driven through every
kernel that uses it: the direct fixed-length kernel, both RALLEDATA forms, the archive prehash
and the import prehash (from the file, and from LDS by the TSV scan).

A key of len bytes is hashed as k = ceil(len / 16) chunks ending at its last byte; chunk 0
starts p = 16 k - len bytes before the key.  The lengths give k = 0..6 with p = 0 and p = 15,
the one-chunk key whose last chunk is also the masked chunk 0, and k = 3, 4, 5 around the
import walker's three chunks in flight.  The placements put a key where chunk 0 would begin
below the buffer (at byte 0 of it, and 1, 7 and 15 bytes in) and where it ends at the buffer's
last byte.  "Buffer" is the pointer handed to the API: a slice 0, 1 or 15 bytes into a torch
allocation, with canary bytes around it that differ between two runs -- no hash may depend on
them.  Every h1 and h2 is compared bit for bit with the oracle (k2h_hash / k2h_second_hash; for
the C-string consumers the oracle hash of key + NUL), never with another device result.
"""
import numpy as np
import pytest

from k2hash_amd import archive, batch, ralledata

LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 81)
STARTS = (0, 1, 7, 15)  # where the first key starts in the buffer
SHIFTS = (0, 1, 15)     # where the buffer starts in its allocation
CANARIES = (0x00, 0xA5)
PAD = 64                # canary bytes on either side of the buffer


def key_bytes(length, salt):
    """Bytes of every sign, none of them TAB, newline or NUL (the TSV scan cuts a key there)."""
    rng = np.random.default_rng(1000 * length + salt)
    b = rng.integers(1, 256, length, dtype=np.uint8)
    b[(b == 9) | (b == 10)] = 0x80
    return b.tobytes()


KEYS = [key_bytes(n, 0) for n in LENGTHS]


def rotated(r):
    return KEYS[r:] + KEYS[:r]


def cases():
    """Every length first in the buffer at every start (and so also last in it, ending at the
    buffer's last byte), the three allocation shifts taken in turn."""
    for r in range(len(KEYS)):
        for j, s in enumerate(STARTS):
            yield rotated(r), s, SHIFTS[(r + j) % len(SHIFTS)]


def place(cuda, payload, shift, canary):
    """payload as a device buffer that starts `shift` bytes into its allocation and ends at the
    payload's last byte, with PAD canary bytes before and after."""
    import torch
    a = np.full(PAD + shift + len(payload) + PAD, canary, np.uint8)
    a[PAD + shift:PAD + shift + len(payload)] = np.frombuffer(payload, np.uint8)
    t = torch.from_numpy(a).to(cuda)
    return t[PAD + shift:PAD + shift + len(payload)]


@pytest.fixture(scope="module")
def want(oracle):
    """(h1, h2) of a key as stored; cached, the oracle is asked once per distinct key."""
    cache = {}

    def f(key):
        if key not in cache:
            cache[key] = (oracle.k2h_hash(key), oracle.k2h_second_hash(key))
        return cache[key]
    return f


def u64s(t):
    return t.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------ fixed-length, direct loads
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 65])
def test_fixed_direct(cuda, want, n):
    """k2h_amd_hash_fixed with 33 <= key_len <= 127 (fnv_fixed_long_kernel, DIRECT): key 0 sits
    at byte 0 of the buffer, key n-1 ends at its last byte, the keys between start at every
    residue the length gives."""
    for key_len in [x for x in LENGTHS if 33 <= x <= 127]:
        keys = [key_bytes(key_len, 1 + i) for i in range(n)]
        for shift in SHIFTS:
            got = []
            for canary in CANARIES:
                buf = place(cuda, b"".join(keys), shift, canary)
                h1, h2 = batch.hash_fixed(buf, key_len, second=True)
                got.append((u64s(h1), u64s(h2)))
            for a, b in got:
                for i, k in enumerate(keys):
                    assert (int(a[i]), int(b[i])) == want(k), (key_len, n, shift, i)


# ------------------------------------------------------------------------------- RALLEDATA
def ralle_hashes(cuda, keys, start, shift, canary, val_len):
    import torch
    koff = np.zeros(len(keys) + 1, np.int64)
    koff[0] = start
    koff[1:] = start + np.cumsum([len(k) for k in keys])
    kbuf = place(cuda, bytes(start) + b"".join(keys), shift, canary)
    vals = torch.full((max(val_len * len(keys), 1),), 0x5A, dtype=torch.uint8, device=cuda)
    voff = torch.arange(len(keys) + 1, dtype=torch.int64, device=cuda) * val_len
    blobs, boff = ralledata.build_ralledata(kbuf, torch.from_numpy(koff).to(cuda), vals, voff)
    blobs, boff = blobs.cpu().numpy(), boff.cpu().numpy()
    out = []
    for i, k in enumerate(keys):
        b = ralledata.parse_blob(blobs[boff[i]:boff[i + 1]].tobytes())
        assert b.key == k, (i, len(k))
        out.append((b.hash, b.subhash))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form,val_len", [("staged", 3), ("group", 256)])
def test_ralledata(cuda, want, form, val_len):
    """k2h_amd_build_ralledata over 64 records whose keys cycle through the lengths: with
    3-byte values the block is staged in LDS (staged_key_hash), with 256-byte values its 16 KiB
    exceed the 12 KiB stage and it takes the group form (global_key_hash, whose lower bound is
    the key buffer's start).  The 16 hash bytes of each blob header are compared."""
    for keys17, start, shift in cases():
        keys = [keys17[i % len(keys17)] for i in range(64)]
        got = [ralle_hashes(cuda, keys, start, shift, c, val_len) for c in CANARIES]
        for run in got:
            for i, k in enumerate(keys):
                assert run[i] == want(k), (form, len(keys17[0]), start, shift, i, len(k))


# ---------------------------------------------------------------------------- archive prehash
@pytest.mark.gpu
def test_archive_prehash(cuda, want):
    """k2h_amd_archive_prehash over caller-supplied records: record i's key is key i; the odd
    ones are SCOM_RENAME records whose new key (exdata) is key i+1, so new_h1 / new_h2 walk the
    same matrix."""
    import torch
    for keys, start, shift in cases():
        n = len(keys)
        offs = start + np.concatenate([[0], np.cumsum([len(k) for k in keys])])
        rows = np.zeros(n, archive.REC_DTYPE)
        for i in range(n):
            j = (i + 1) % n
            rows["type"][i] = archive.SCOM_RENAME if i & 1 else archive.SCOM_SET_ALL
            rows["key_off"][i], rows["key_len"][i] = offs[i], len(keys[i])
            rows["exdata_off"][i], rows["exdata_len"][i] = offs[j], len(keys[j])
        t = torch.from_numpy(rows.view(np.int64).reshape(-1, archive.REC_WORDS).copy()).to(cuda)
        got = []
        for canary in CANARIES:
            file = place(cuda, bytes(start) + b"".join(keys), shift, canary)
            got.append([u64s(x) for x in archive.prehash_device(file, t, rename=True)])
        for h1, h2, nh1, nh2 in got:
            for i in range(n):
                what = (len(keys[0]), start, shift, i, len(keys[i]))
                assert (int(h1[i]), int(h2[i])) == want(keys[i]), what
                new = want(keys[(i + 1) % n]) if i & 1 else (0, 0)
                assert (int(nh1[i]), int(nh2[i])) == new, what


# ----------------------------------------------------------------------------- import prehash
@pytest.mark.gpu
def test_import_prehash(cuda, want):
    """k2h_amd_import_prehash over caller-supplied records (hash_cstr_unchecked, reading the
    file): each key is hashed as the C string key + NUL."""
    import torch
    for keys, start, shift in cases():
        n = len(keys)
        offs = start + np.concatenate([[0], np.cumsum([len(k) for k in keys])])
        rows = np.zeros((n, 4), np.int64)
        rows[:, 0], rows[:, 1] = offs[:n], [len(k) for k in keys]
        t = torch.from_numpy(rows).to(cuda)
        got = []
        for canary in CANARIES:
            file = place(cuda, bytes(start) + b"".join(keys), shift, canary)
            got.append([u64s(x) for x in archive.import_prehash_device(file, t)])
        for h1, h2 in got:
            for i, k in enumerate(keys):
                assert (int(h1[i]), int(h2[i])) == want(k + b"\0"), (len(keys[0]), start, shift, i, len(k))


@pytest.mark.gpu
def test_import_scan_hashes_keys_from_lds(cuda, want):
    """The TSV scan hashes its keys from the block's LDS image (key_raw_lds): a file of
    key TAB value lines whose keys have the matrix lengths, each length first in the file once.
    The records say which bytes were hashed; the hashes are the oracle's of those bytes + NUL."""
    for r in range(len(KEYS)):
        keys = rotated(r)
        data = b"".join(k + b"\tv%d\n" % i for i, k in enumerate(keys))
        shift = SHIFTS[r % len(SHIFTS)]
        got = []
        for canary in CANARIES:
            file = place(cuda, data, shift, canary)
            recs, h1, h2 = archive.import_scan_prehash_device(file, "tsv")
            got.append((recs.cpu().numpy(), u64s(h1), u64s(h2)))
        for recs, h1, h2 in got:
            assert [bytes(data[o:o + n]) for o, n in recs[:, :2]] == keys, r
            for i, k in enumerate(keys):
                assert (int(h1[i]), int(h2[i])) == want(k + b"\0"), (r, shift, i, len(k))


def test_matrix_covers_the_walkers_paths():
    """Chunk counts 0..6, both extremes of the lead pad, and a key of every length that starts
    closer to the buffer's start than its pad (the bytes-only chunk 0)."""
    ks = {(n + 15) // 16 for n in LENGTHS}
    assert ks == set(range(7))
    pads = {16 * ((n + 15) // 16) - n for n in LENGTHS if n}
    assert {0, 15} <= pads
    assert all(any(s < p for s in STARTS) for p in pads if p)
