"""CPU test of the screened shared-row scan with row-level admission
(scan_f32_qshare_screen_kernel, wvg_qshare.hip) from the built library's gfx950
kernel descriptor: the kernel exists once, uses no private memory, stays within
the 256 registers of two waves per SIMD, and its LDS (the combine buffer, the
bf16 and the fp32 query images) leaves room for two workgroups per CU."""
import os
import re
import subprocess

from test_capi import _gfx950_code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KEYS = (".private_segment_fixed_size", ".vgpr_count", ".group_segment_fixed_size")
LDS_PER_CU = 160 * 1024


def _kernels(tmp_path, pattern):
    """{kernel name: {metadata key: value}} of the library's kernels whose mangled name matches."""
    from weaviate_amd import _lib

    found = {}
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"qsr{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        # a kernel's metadata block: its keys are sorted, .name lies between .agpr_count and .vgpr_count
        for block in notes.split("- .agpr_count:")[1:]:
            m = re.search(r"\.name:\s+(\S+)", block)
            if not m or not re.search(pattern, m.group(1)):
                continue
            found[m.group(1)] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", block).group(1)) for k in KEYS}
    return found


def test_row_admission_scan_fits_two_workgroups_per_cu(tmp_path):
    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain that built the library"
    scan = _kernels(tmp_path, r"\d+scan_f32_qshare_screen_kernelE")
    assert len(scan) == 1, sorted(scan)
    (name, md), = scan.items()
    assert md[".private_segment_fixed_size"] == 0, (name, md)
    assert md[".vgpr_count"] <= 256, (name, md)
    assert md[".group_segment_fixed_size"] <= 80 * 1024 and 2 * md[".group_segment_fixed_size"] <= LDS_PER_CU, (name, md)
