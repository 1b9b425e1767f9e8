"""CPU: the host WebP decoder (csrc/webp_host.cpp, plain C++) under AddressSanitizer + UBSan on mutated files - truncations
and cut spans with the container sizes made right again (so the bit reader, not the chunk walk, meets the damage), bit
flips, corrupted headers - of Pillow-encoded and hand-written files: every transform, colour cache, meta prefix image,
backward references.  The harness is a stand-alone program run as a child process; any out-of-bounds access aborts it."""
import os
import shutil
import subprocess

import pytest

from tests import _webp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_webp_decoder_survives_mutated_streams(tmp_path):
    exe = tmp_path / "webp_fuzz"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           f"-I{ROOT}/include", os.path.join(ROOT, "tests", "fuzz", "webp_fuzz.cpp"),
           os.path.join(ROOT, "vip-cup-2022_amd", "csrc", "webp_host.cpp"), "-o", str(exe), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    files = []
    for name, raw in _webp.corpus(seed=9, sizes=[(3, 5), (17, 13), (65, 7)])[::5]:
        p = tmp_path / f"{name}.webp"
        p.write_bytes(raw)
        files.append(str(p))
    r = subprocess.run([str(exe), "150", *files], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0"})
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
    assert "fuzzed" in r.stdout
    n_total, n_ok = int(r.stdout.split()[1]), int(r.stdout.split()[3])
    assert n_total > 5000 and 0 < n_ok < n_total          # some mutations still decode, most are rejected or cut short
