"""The grouped PQ kernels (wvg_group_pq.hip) in the built library's gfx950 descriptors: both exist, none
uses private memory, and the scan's compiled (E, NC, GL) forms are those tests/test_gpu_group_pq.py runs."""
import re
import subprocess

from test_capi import _gfx950_code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def test_group_pq_kernels_use_no_scratch_and_match_the_gpu_matrix(tmp_path):
    from test_gpu_group_pq import kernel_forms
    from weaviate_amd import _lib

    private = {}  # "lut" / (E, NC, GL) -> private segment bytes
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"gpq{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        name = None
        for ln in notes.splitlines():
            ln = ln.strip()
            if ln.startswith(".name:"):
                m = re.search(r"\d+scan_pq_group_kernelILi(\d+)ELi(\d+)ELb([01])EE", ln)
                name = (int(m.group(1)), int(m.group(2)), m.group(3) == "1") if m else None
                if re.search(r"\d+pq_lut_group_kernelE", ln):
                    name = "lut"
            elif ln.startswith(".private_segment_fixed_size:") and name is not None:
                private[name] = int(ln.split(":", 1)[1])
                name = None
    assert "lut" in private, "the library holds no pq_lut_group_kernel"
    assert not {k: v for k, v in private.items() if v != 0}, private
    scan = set(private) - {"lut"}
    assert scan == kernel_forms(), sorted(scan ^ kernel_forms(), key=str)
