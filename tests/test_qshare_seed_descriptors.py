"""CPU test of the shared-row scan's prologue (qshare_seed_kernel, wvg_qshare.hip)
from the built library's gfx950 kernel descriptors: the forms
wvg_search_device_pipelined launches all exist, none uses private memory, and
their names stay clear of the substring the bench and the traffic profile use
to find the scan kernel."""
import os
import re
import subprocess

from test_capi import _gfx950_code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def _seed_kernels(tmp_path):
    """{(metric, D, E): private_segment_fixed_size} of the library's qshare_seed_kernel forms, and their names."""
    from weaviate_amd import _lib

    found, names = {}, []
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"qseed{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        name = None
        for ln in notes.splitlines():
            ln = ln.strip()
            if ln.startswith(".name:"):
                m = re.search(r"\d+qshare_seed_kernelILi(\d+)ELi(\d+)ELi(\d+)EE", ln)
                name = tuple(int(x) for x in m.groups()) if m else None
                if m:
                    names.append(ln)
            elif ln.startswith(".private_segment_fixed_size:") and name:
                found[name] = int(ln.split(":", 1)[1])
                name = None
    return found, names


def test_seed_kernels_exist_and_use_no_scratch(tmp_path):
    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain that built the library"
    found, names = _seed_kernels(tmp_path)
    want = {(metric, d, e) for metric in (0, 1) for d in (128, 768) for e in (1, 2, 4)}  # L2 / dot (cosine runs dot)
    assert want <= set(found), sorted(want - set(found))
    spilled = {k: v for k, v in found.items() if v != 0}
    assert not spilled, spilled
    assert not [n for n in names if "scan_f32_qshare" in n], names
