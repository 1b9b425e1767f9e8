"""CPU: the fused fp16 MLP kernels (csrc/mlp_fused.hip) that vip_mlp_fused_supported can select keep everything in registers.
mlp_stream_kernel prefetches the next hidden slice's weights global -> VGPR at the head of a slice and writes them to LDS at its tail;
held in an array, hipcc left those staging values on the stack (48 / 64 bytes of scratch per lane at C = 128 / 192 with no register
spilled: a second memory round trip in every slice), so they are named scalars now.  mlp_fused_kernel at C = 96 sits at the 128
registers that four waves per SIMD allow, and what keeps it there is an opaque copy of a lane index at the tile head.  A compiler
update, or an edit of either loop, can undo both silently, and a loop that goes through scratch is slower without being wrong.
csrc/mlp_fused.hip is compiled for the device alone with the flags of the build, the way tools/kernel_resources.py does it, and only
the compiler's resource remarks are read; nothing runs on a GPU.  mlp_stream_kernel<8,3> (C = 256) is built but not offered and may
keep scratch: it is listed, not held."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# kernel, template arguments -> VGPR budget; the instantiations behind C = 64, 96 (LDS-resident weights) and C = 128, 192 (streamed)
HELD = {("mlp_fused_kernel", (2, 3, 2)): 128, ("mlp_fused_kernel", (3, 3, 2)): 128,
        ("mlp_stream_kernel", (4, 3)): 256, ("mlp_stream_kernel", (6, 3)): 256}
NOT_OFFERED = {("mlp_stream_kernel", (8, 3))}


def _hipcc():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import build
    return build


def _have_hipcc():
    try:
        return os.path.exists(_hipcc().HIPCC)
    except Exception:
        return False


@pytest.mark.skipif(not _have_hipcc(), reason="no hipcc in this image")
def test_mlp_kernels_stay_in_registers():
    build = _hipcc()
    src = os.path.join(build.CSRC, "mlp_fused.hip")
    cmd = [build.HIPCC, *build.CXXFLAGS, *build.EXTRA_FLAGS.get("mlp_fused.hip", []), "--cuda-device-only", "-x", "hip", "-c", src,
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(":")
        if key.strip() == "Function Name":
            t = re.search(r"\d+(mlp_fused_kernel|mlp_stream_kernel)I((?:Li\d+E)+)E", val)
            cur = seen.setdefault((t.group(1), tuple(int(v) for v in re.findall(r"Li(\d+)E", t.group(2)))), {}) if t else None
        elif cur is not None:
            cur[key.strip()] = val.strip()
    assert set(seen) == set(HELD) | NOT_OFFERED, sorted(seen)                # the remarks really listed every instantiation
    for inst, res in sorted(seen.items()):
        print(f"{inst[0]}{inst[1]}: VGPRs {res['VGPRs']}, spilled {res['VGPRs Spill']}, SGPRs spilled {res['SGPRs Spill']}, "
              f"scratch {res['ScratchSize [bytes/lane]']} B/lane, {res['Occupancy [waves/SIMD]']} waves/SIMD")
    bad = {inst: res for inst, res in seen.items() if inst in HELD and
           (int(res["ScratchSize [bytes/lane]"]) != 0 or int(res["VGPRs Spill"]) != 0 or int(res["SGPRs Spill"]) != 0
            or int(res["VGPRs"]) > HELD[inst])}
    assert not bad, bad
