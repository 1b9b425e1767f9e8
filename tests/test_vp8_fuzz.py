"""CPU: the host half of the lossy WebP path (csrc/vp8_host.cpp, plain C++) under AddressSanitizer + UBSan on mutated files -
truncations and cut spans with the RIFF, chunk and first-partition sizes made right again (so the boolean decoder, not the
container walk, meets the damage), bit flips, corrupted headers - of Pillow-encoded files, the fixtures and hand-written key
frames: segments, 1-8 partitions, sub-block modes, every token category.  The harness is a stand-alone program run as a child
process; any out-of-bounds access aborts it, and so does a record the device could not index with."""
import os
import shutil
import subprocess

import pytest

from tests import _vp8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_vp8_decoder_survives_mutated_streams(tmp_path):
    exe = tmp_path / "vp8_fuzz"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           f"-I{ROOT}/include", os.path.join(ROOT, "tests", "fuzz", "vp8_fuzz.cpp"),
           os.path.join(ROOT, "vip-cup-2022_amd", "csrc", "vp8_host.cpp"), "-o", str(exe), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    files = []
    corp = [(n, raw) for n, raw in _vp8.corpus(1) if len(raw) < 3000]
    for name, raw in corp[::4] + [c for c in corp if c[0].startswith(("fx_", "hw_"))][::2]:
        p = tmp_path / f"{name}.webp"
        p.write_bytes(raw)
        files.append(str(p))
    r = subprocess.run([str(exe), "250", *files], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0"})
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
    assert "fuzzed" in r.stdout
    n_total, n_ok = int(r.stdout.split()[1]), int(r.stdout.split()[3])
    assert n_total > 5000 and 0 < n_ok < n_total          # some mutations still decode, most are rejected or cut short
