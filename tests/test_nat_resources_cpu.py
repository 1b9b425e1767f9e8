"""CPU: no kernel of csrc/nat_attn.hip spills.  The fp16 kernel holds a Q fragment, thirty-two score accumulators, eight K fragments and
the P / V fragments of a query tile per lane, the fp32 template a 32-element query and a 32-element output row per thread; a spill
would put them in scratch without making anything wrong.  The file is compiled for the device alone with the flags of the build, the
way tests/test_swin_resources_cpu.py compiles swin_attn.hip, and only the compiler's resource remarks are read; nothing runs on a GPU."""
import os
import re
import subprocess

import pytest

KERNELS = {"nat_attn_kernel", "nat_attn_strict_kernel<NA32>", "nat_attn_strict_kernel<NAH2>"}
# read from the first compile of the file: 90 VGPRs, 29376 bytes of LDS per four-wave workgroup.  Up to 96 registers five waves fit a
# SIMD, and the LDS admits five workgroups (20 waves) per compute unit: the two limits meet.
VGPR_CEILING = 96


def _build():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import build
    return build


def _have_hipcc():
    try:
        return os.path.exists(_build().HIPCC)
    except Exception:
        return False


@pytest.mark.skipif(not _have_hipcc(), reason="no hipcc in this image")
def test_nat_attn_kernels_do_not_spill():
    build = _build()
    src = os.path.join(build.CSRC, "nat_attn.hip")
    assert src in build._sources()
    cmd = [build.HIPCC, *build.CXXFLAGS, *build.EXTRA_FLAGS.get("nat_attn.hip", []), "--cuda-device-only", "-x", "hip", "-c", src,
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
            t = re.search(r"nat_attn_(strict_)?kernel(?:INS_\d+(NA\w+?)EEE)?", val)
            name = None if not t else ("nat_attn_kernel" if not t.group(1) else f"nat_attn_strict_kernel<{t.group(2)}>")
            cur = seen.setdefault(name, {}) if name else None
        elif cur is not None:
            cur[key.strip()] = val.strip()
    assert set(seen) == KERNELS, sorted(seen)                          # the remarks really listed every kernel
    for name, res in sorted(seen.items()):
        print(f"{name}: VGPRs {res['VGPRs']}, spilled {res['VGPRs Spill']}, scratch {res['ScratchSize [bytes/lane]']} B/lane, "
              f"LDS {res['LDS Size [bytes/block]']} B, {res['Occupancy [waves/SIMD]']} waves/SIMD")
    bad = {n: res for n, res in seen.items() if int(res["VGPRs Spill"]) != 0 or int(res["ScratchSize [bytes/lane]"]) != 0}
    assert not bad, bad
    assert int(seen["nat_attn_kernel"]["VGPRs"]) <= VGPR_CEILING
    assert int(seen["nat_attn_kernel"]["LDS Size [bytes/block]"]) * 5 <= 160 * 1024     # five workgroups per compute unit
