"""CPU test of the screened shared-row scan (scan_f32_qshare_screen_kernel) and its
extended prologue (qshare_seed_kernel<L2, 128, E>, which also writes the queries'
bf16 images and bound constants; wvg_qshare.hip) from the built library's gfx950
kernel descriptors: both exist, use no private memory and stay within the 256
registers of two waves per SIMD."""
import os
import re
import subprocess

from test_capi import _gfx950_code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KEYS = (".private_segment_fixed_size", ".vgpr_count", ".agpr_count")


def _kernels(tmp_path, pattern):
    """{kernel name: {metadata key: value}} of the library's kernels whose mangled name matches."""
    from weaviate_amd import _lib

    found = {}
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"qsc{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        # a kernel's metadata block: its keys are sorted, .name lies between .agpr_count and .vgpr_count
        for block in notes.split("- .agpr_count:")[1:]:
            block = ".agpr_count:" + block
            m = re.search(r"\.name:\s+(\S+)", block)
            if not m or not re.search(pattern, m.group(1)):
                continue
            found[m.group(1)] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", block).group(1)) for k in KEYS}
    return found


def test_screened_scan_and_prologue_fit_two_waves_per_simd(tmp_path):
    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain that built the library"
    scan = _kernels(tmp_path, r"\d+scan_f32_qshare_screen_kernelE")
    assert len(scan) == 1, sorted(scan)
    seed = _kernels(tmp_path, r"\d+qshare_seed_kernelILi0ELi128ELi[124]EE")
    assert len(seed) == 3, sorted(seed)
    for name, md in {**scan, **seed}.items():
        assert md[".private_segment_fixed_size"] == 0, (name, md)
        assert md[".vgpr_count"] <= 256 and md[".agpr_count"] <= md[".vgpr_count"], (name, md)  # .vgpr_count: both files
