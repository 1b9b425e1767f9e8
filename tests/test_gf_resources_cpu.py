"""CPU: no instantiation of global_local_filter_kernel<storage, W> (csrc/global_filter.hip) spills.  The register-blocked widths hold
W x 4 accumulators and W x 4 source values per lane (W = 14: 112 of them) next to nine 3x3 taps; a spill would put the inner product's
operands in scratch without making anything wrong.  The file is compiled for the device alone with the flags of the build, the way
tests/test_dw_resources_cpu.py compiles dwconv.hip, and only the compiler's resource remarks are read; nothing runs on a GPU."""
import os
import re
import subprocess

import pytest

# every (storage, W) the launcher can select: the four specialised widths and the generic form (W = 0), on the three storages
INSTANTIATIONS = {(s, w) for s in ("GF16", "GF32", "GH2") for w in (14, 12, 7, 6, 0)}


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
def test_global_filter_kernels_do_not_spill():
    build = _build()
    src = os.path.join(build.CSRC, "global_filter.hip")
    text = open(src).read()
    assert {int(w) for w in re.findall(r"case (\d+): GF_LAUNCH\(\1\)", text)} | {0} == {w for _, w in INSTANTIATIONS}
    assert "default: GF_LAUNCH(0)" in text
    cmd = [build.HIPCC, *build.CXXFLAGS, *build.EXTRA_FLAGS.get("global_filter.hip", []), "--cuda-device-only", "-x", "hip", "-c", src,
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
            t = re.search(r"global_local_filter_kernelINS_\d+(G\w+?)ELi(\d+)EEE", val)
            cur = seen.setdefault((t.group(1), int(t.group(2))), {}) if t else None
        elif cur is not None:
            cur[key.strip()] = val.strip()
    assert set(seen) == INSTANTIATIONS, sorted(seen)                   # the remarks really listed every instantiation
    for inst, res in sorted(seen.items()):
        print(f"global_local_filter_kernel{inst}: VGPRs {res['VGPRs']}, spilled {res['VGPRs Spill']}, scratch "
              f"{res['ScratchSize [bytes/lane]']} B/lane, {res['Occupancy [waves/SIMD]']} waves/SIMD")
    bad = {inst: res for inst, res in seen.items() if int(res["VGPRs Spill"]) != 0 or int(res["ScratchSize [bytes/lane]"]) != 0}
    assert not bad, bad
