"""The index layout of k2h_find_layout.h (CPU only): k2h_amd_ralledata_index_size equals the
layout's measured total, the measuring and the placing pass agree, and the columns are the ones
include/k2hash_amd.h section 4e names -- a 256-byte header, 8 + 4 + 32 bytes per blob, each
column 256-byte aligned.  tests/find_layout_probe.cc is built with the host compiler alone.
"""
import subprocess

import pytest

from test_scratch_layout import CSRC, ROOT, _compiler, align256

from k2hash_amd import _native

NS = [0, 1, 255, 256, 257, (1 << 20) + 3, (1 << 32) - 2]
PROBE = ROOT / "tests" / "find_layout_probe.cc"


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("find_layout") / "probe"
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(PROBE), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe), *map(str, NS)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return [ln.split() for ln in r.stdout.splitlines()]


def test_size_function_is_the_layout(probe):
    lib = _native.batch_lib()
    assert [w for w in probe if w[0] == "header"] == [["header", "48", "256", "32"]]
    for n in NS:
        measure, place = ([int(x) for x in w[3:]] for w in probe if w[0] == "cols" and int(w[1]) == n)
        assert measure == place
        head, hash_, idx, side, total = measure
        assert (head, hash_) == (0, 256) and idx == hash_ + align256(8 * n) and side == idx + align256(4 * n)
        assert total == side + align256(32 * n)
        assert lib.k2h_amd_ralledata_index_size(n) == total, n
        assert 44 * n + 256 <= total <= 44 * n + 256 + 3 * 255


def test_layout_header_needs_no_hip():
    text = (CSRC / "k2h_find_layout.h").read_text()
    assert "hip" not in text.lower()
