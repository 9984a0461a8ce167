"""CPU test of the packed-round form of the shadow-fed shared-row scan (scan_f32_qshare_shadow_kernel and
its filtered twin; wvg_qshare.hip, "Packed rounds") from the built library's gfx950 kernel descriptors.
The waves' pending queues live in LDS beside the fp32 query image and the combine buffer, and the kernel
is built for two waves per SIMD, that is two workgroups of four waves per CU: both kernels use no private
memory, stay within 256 registers, and two workgroups' LDS fits a CU's 160 KiB."""
import os
import re
import subprocess

from test_capi import _gfx950_code_objects
from test_qshare_screen_descriptors import READELF

KEYS = (".private_segment_fixed_size", ".vgpr_count", ".agpr_count", ".group_segment_fixed_size")
CU_LDS = 160 * 1024
QUEUES = 4 * (63 + 16 * 64) * 4  # four waves' queues of 32-bit entries: the least the kernel must hold


def _kernels(tmp_path, pattern):
    from weaviate_amd import _lib

    found = {}
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"qsp{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            block = ".agpr_count:" + block
            m = re.search(r"\.name:\s+(\S+)", block)
            if not m or not re.search(pattern, m.group(1)):
                continue
            found[m.group(1)] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", block).group(1)) for k in KEYS}
    return found


def test_packed_shadow_kernels_fit_two_workgroups_per_cu(tmp_path):
    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain that built the library"
    plain = _kernels(tmp_path, r"\d+scan_f32_qshare_shadow_kernelE")
    filt = _kernels(tmp_path, r"\d+scan_f32_qshare_shadow_filt_kernelE")
    assert len(plain) == 1, sorted(plain)
    assert len(filt) == 1, sorted(filt)
    for name, md in {**plain, **filt}.items():
        print(name, md)
        assert md[".private_segment_fixed_size"] == 0, (name, md)
        assert md[".vgpr_count"] <= 256 and md[".agpr_count"] <= md[".vgpr_count"], (name, md)
        assert 2 * md[".group_segment_fixed_size"] <= CU_LDS, (name, md)
        assert md[".group_segment_fixed_size"] >= QUEUES, (name, md)  # the queues are there
