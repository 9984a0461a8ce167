"""CPU test of the shared-row query-stream kernels (scan_f32_qshare_kernel,
wvg_qshare.hip) from the built library's gfx950 kernel descriptors: no
instantiation uses private memory (a spilled register or a dynamically indexed
per-query top-k state would: DESIGN.md section 5, "A scratch regression"), and
the forms wvg_search_device_pipelined routes to all exist."""
import os
import re
import subprocess

from test_capi import _gfx950_code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def _qshare_kernels(tmp_path):
    """{(metric, D, E, whole): private_segment_fixed_size} of the library's scan_f32_qshare_kernel forms."""
    from weaviate_amd import _lib

    found = {}
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"qs{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        name = None
        for ln in notes.splitlines():
            ln = ln.strip()
            if ln.startswith(".name:"):
                m = re.search(r"\d+scan_f32_qshare_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])EE", ln)
                name = tuple(int(x) for x in m.groups()) if m else None
            elif ln.startswith(".private_segment_fixed_size:") and name:
                found[name] = int(ln.split(":", 1)[1])
                name = None
    return found


def test_qshare_kernels_exist_and_use_no_scratch(tmp_path):
    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain that built the library"
    found = _qshare_kernels(tmp_path)
    forms = {(metric, d, e) for metric, d, e, _ in found}
    want = {(metric, d, e) for metric in (0, 1) for d in (128, 768) for e in (1, 2, 4)}  # L2 / dot (cosine runs dot)
    assert want <= forms, sorted(want - forms)
    spilled = {k: v for k, v in found.items() if v != 0}
    assert not spilled, spilled
