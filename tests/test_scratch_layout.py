"""The launchers' shared layout header, k2h_layout.h, on the host alone (CPU only).

tests/scratch_layout_probe.cc is built against the header with the host compiler, once plainly
and once with the address and undefined-behaviour sanitizers, and run as a child process; what
it prints is checked here.  A second test reads the sources: the scratch type, the helpers and
the size of a launcher's buffer are each written in one place.
"""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "k2hash_amd" / "csrc"
PROBE = ROOT / "tests" / "scratch_layout_probe.cc"
SHARED = ("k2h_layout.h", "k2h_scratch.h")

SORT_NS = [1, 2, 255, 256, 257, 65535, 65536, 65537, 1 << 24, (1 << 24) + 1, (1 << 32) - 2, (1 << 56) + 1]
# the probe's columns: name, bytes; "rec16" only in the variant with the trailing column
COLUMNS = [("u64", 37 * 8), ("u32", 101 * 4), ("rec32", 9 * 32), ("empty", 0), ("u8", 300), ("u16", 129 * 2),
           ("tmp", 1000), ("counter", 4096)]
TRAILING = ("rec16", 5 * 16)


def sort_bits_for(n):
    """k2h_layout.h's, transliterated."""
    bits = 0
    while bits < 64 and (n - 1) >> bits:
        bits += 1
    bits = (bits + 8 + 7) // 8 * 8
    return 16 if bits < 16 else 64 if bits > 64 else bits


def sort_mask(bits):
    return (1 << 64) - 1 if bits == 64 else (1 << bits) - 1


def align256(x):
    return (x + 255) & ~255


def _compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    pytest.skip("no host C++ compiler")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    """The probe's output lines, split into words."""
    exe = tmp_path_factory.mktemp("layout") / f"probe_{request.param}"
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", f"-I{CSRC}"]
    cxx = _compiler()
    if request.param == "sanitized":
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
        # the runtimes linked into the program (clang's default), so that it runs as it is wherever
        # the suite runs
        if "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
            flags += ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, *flags, str(PROBE), "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert not r.stderr, r.stderr
    return [ln.split() for ln in r.stdout.splitlines()]


def test_sort_bits_and_mask(probe):
    got = {int(w[1]): (int(w[2]), int(w[3], 16)) for w in probe if w[0] == "bits"}
    assert sorted(got) == sorted(SORT_NS)
    for n in SORT_NS:
        bits = sort_bits_for(n)
        assert got[n] == (bits, sort_mask(bits)), n
    assert got[1][0] == 16 and got[(1 << 24) + 1][0] == 40 and got[(1 << 32) - 2][0] == 40
    assert got[(1 << 56) + 1] == (64, (1 << 64) - 1)


@pytest.mark.parametrize("trailing", [0, 1])
def test_measure_and_place_agree(probe, trailing):
    want = COLUMNS + ([TRAILING] if trailing else [])
    passes = {}
    for name in ("measure", "place"):
        cols = [(w[3], int(w[4]), int(w[5]), int(w[6])) for w in probe
                if w[0] == "col" and int(w[1]) == trailing and w[2] == name]
        total = [int(w[3]) for w in probe if w[0] == "total" and int(w[1]) == trailing and w[2] == name]
        assert len(total) == 1
        passes[name] = (cols, total[0])
    assert passes["measure"] == passes["place"]  # offsets, sizes and total; the placed base is aligned
    cols, total = passes["place"]
    assert [(c[0], c[2]) for c in cols] == want
    end = 0
    for name, off, size, misalign in cols:
        assert off % 256 == 0 and misalign == 0, name
        assert off == end, name  # consecutive: neither an overlap nor a gap beyond the alignment
        end = off + align256(size)
    assert total == end  # the end of the last column
    by_name = {c[0]: c for c in cols}
    nxt = cols[[c[0] for c in cols].index("empty") + 1]
    assert by_name["empty"][1] == nxt[1] and by_name["empty"][1] <= total  # takes no space, points into the buffer
    if not trailing:
        assert "rec16" not in by_name


def test_trailing_column_only_adds_to_the_end(probe):
    def cols(t):
        return [w[3:] for w in probe if w[0] == "col" and int(w[1]) == t and w[2] == "measure"]
    assert cols(1)[:-1] == cols(0)
    tot = {int(w[1]): int(w[3]) for w in probe if w[0] == "total" and w[2] == "measure"}
    assert tot[1] == tot[0] + align256(TRAILING[1])


def test_counter_line_sum(probe):
    shape = [w for w in probe if w[0] == "counter"]
    assert shape == [["counter", "64", "8", "4096"]]
    got = {int(w[1]): int(w[2]) for w in probe if w[0] == "sum"}
    for word in (0, 6):
        assert got[word] == sum(1000 * (c + 1) + 7 * word * word + word for c in range(64))


def _code(path):
    text = path.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def test_scratch_and_helpers_are_written_once():
    sources = [f for f in sorted(CSRC.iterdir()) if f.suffix in (".hip", ".cc", ".h", ".inc")]
    assert {f.name for f in sources} >= set(SHARED)
    reserves = 0
    for f in sources:
        code = _code(f)
        if f.name in SHARED:
            continue
        assert not re.search(r"\b(align256|sort_bits_for)\s*\([^()]*\)\s*\{", code), f.name
        for m in re.finditer(r"\bstruct\s+(\w*Scratch)\b[^{;]*\{(.*?)\n\};", code, flags=re.S):
            body = m.group(2)
            own = [x for x in (r"\bstd::mutex\s+mu\b", r"\bvoid\s*\*\s*p\b", r"\bsize_t\s+bytes\b") if re.search(x, body)]
            assert not own, (f.name, m.group(1), own)
        assert not re.search(r"\btotal\s*=[^;]*\balign256\b", code), f.name
        # a buffer's size is what the layout measured, never a sum written next to it
        for m in re.finditer(r"(?:\.|->)(?:reserve|grow)\s*\(\s*([^,]*),", code):
            assert m.group(1).strip() == "layout(nullptr).total", (f.name, m.group(0))
            reserves += 1
    assert reserves >= 11  # select, partition, fold, dedup, diff, subkeys x2, reach, unlink, two scanners
    layout = _code(CSRC / "k2h_layout.h")
    assert "hip" not in layout.lower()
