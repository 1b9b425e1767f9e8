"""CPU: the LayerNorm-prologue GEMM instantiations (pwx_ln_kernel<2|3|4|6, 2>) carry no scratch.  What keeps the K = 384 instantiation
(96 fragment + 64 accumulator registers) out of scratch are hand-placed opaque statements in its prologue (csrc/conv_igemm.hip): a
compiler update can undo them silently, and a spilling prologue is slower without being wrong.  The kernel metadata
(.private_segment_fixed_size, .vgpr_count) is read from the code objects of the built library with llvm-readelf; nothing runs on a GPU."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-objdump") or not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm tools in this image")
def test_ln_gemm_kernels_have_no_scratch():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import build
    lib = build.build_lib()
    tmp = tempfile.mkdtemp(prefix="ln_gemm_res_")
    try:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(lib, so)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", so], capture_output=True, text=True, check=True)
        seen = {}
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", os.path.join(tmp, f)], capture_output=True, text=True, check=True).stdout
            for blk in re.split(r"\n\s*- \.agpr_count:", notes):       # one block per kernel of amdhsa.kernels
                name = re.search(r"\.name:\s+(\S*pwx_ln_kernel\S*)", blk)
                if not name:
                    continue
                seen[name.group(1)] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                                       int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                                       int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kscs = sorted(int(re.search(r"pwx_ln_kernelILi(\d+)ELi2E", k).group(1)) for k in seen)
    assert kscs == [2, 3, 4, 6], seen                                  # the metadata really listed every instantiation
    assert all(v == (0, v[1], 0) and v[1] <= 256 for v in seen.values()), seen
