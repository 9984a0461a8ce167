"""CPU test of the runtime-dimension shared-row kernels (scan_f32_qshare_dyn_kernel
and scan_f32_qshare_dyn_filt_kernel, wvg_qshare.hip) from the built library's
gfx950 kernel descriptors: both exist for metric in {L2, dot} x E in {1, 2, 4}
(cosine runs dot), and none uses private memory (4 x 32 accumulators live
through a row: a spill or a dynamically indexed per-query state would)."""
import os
import re
import subprocess

from test_capi import _gfx950_code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def _dyn_kernels(tmp_path):
    """{(filtered, metric, E): private_segment_fixed_size} of the library's runtime-dimension forms."""
    from weaviate_amd import _lib

    found = {}
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"qd{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        name = None
        for ln in notes.splitlines():
            ln = ln.strip()
            if ln.startswith(".name:"):
                m = re.search(r"\d+scan_f32_qshare_dyn_(filt_)?kernelILi(\d+)ELi(\d+)EE", ln)
                name = (m.group(1) is not None, int(m.group(2)), int(m.group(3))) if m else None
            elif ln.startswith(".private_segment_fixed_size:") and name:
                found[name] = int(ln.split(":", 1)[1])
                name = None
    return found


def test_dyn_kernels_exist_and_use_no_scratch(tmp_path):
    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain that built the library"
    found = _dyn_kernels(tmp_path)
    want = {(filt, metric, e) for filt in (False, True) for metric in (0, 1) for e in (1, 2, 4)}
    assert want <= set(found), sorted(want - set(found))
    spilled = {k: v for k, v in found.items() if v != 0}
    assert not spilled, spilled
