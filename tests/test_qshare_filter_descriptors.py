"""CPU test of the filtered shared-row kernels (scan_f32_qshare_filt_kernel,
scan_f32_qshare_screen_filt_kernel, qshare_seed_filt_kernel; wvg_qshare.hip)
from the built library's gfx950 kernel descriptors: the forms
wvg_search_device_pipelined_filtered launches all exist, the screened one exactly
once, none has a private segment, every one stays within 256 vector registers
(two waves per SIMD) and twice its LDS fits a CU's 160 KiB (two workgroups per
CU)."""
import os
import re
import subprocess

from test_capi import _gfx950_code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KEYS = (".private_segment_fixed_size", ".vgpr_count", ".group_segment_fixed_size", ".vgpr_spill_count")


def _kernels(tmp_path, pattern):
    """{mangled name: {key: value}} of the library's kernels whose name matches."""
    from weaviate_amd import _lib

    found = {}
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"qfilt{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for block in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
            m = re.search(r"\.name:\s+(\S+)", block)
            if not m or not re.search(pattern, m.group(1)):
                continue
            found[m.group(1)] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", block).group(1)) for k in KEYS}
    return found


def _check(found):
    for name, d in found.items():
        assert d[".private_segment_fixed_size"] == 0 and d[".vgpr_spill_count"] == 0, (name, d)
        assert d[".vgpr_count"] <= 256, (name, d)
        assert 2 * d[".group_segment_fixed_size"] <= 160 * 1024, (name, d)


def test_filtered_scan_kernels(tmp_path):
    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain that built the library"
    found = _kernels(tmp_path, r"\d+scan_f32_qshare_filt_kernelILi\d+ELi\d+ELi\d+ELb[01]EE")
    forms = set()
    for name in found:
        m = re.search(r"scan_f32_qshare_filt_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])EE", name)
        forms.add(tuple(int(x) for x in m.groups()))
    # L2 / dot (cosine runs dot); whole rows at d = 128, blocks at d = 768; E = 1, 2, 4
    want = {(metric, d, e, int(d == 128)) for metric in (0, 1) for d in (128, 768) for e in (1, 2, 4)}
    assert want <= forms, sorted(want - forms)
    _check(found)


def test_filtered_screen_kernel_exists_once(tmp_path):
    found = _kernels(tmp_path, r"\d+scan_f32_qshare_screen_filt_kernelE")
    assert len(found) == 1, sorted(found)
    _check(found)
    # the unfiltered screened kernel is still the only kernel of its name
    assert len(_kernels(tmp_path, r"\d+scan_f32_qshare_screen_kernelE")) == 1


def test_filtered_seed_kernels(tmp_path):
    found = _kernels(tmp_path, r"\d+qshare_seed_filt_kernelILi\d+ELi\d+ELi\d+EE")
    forms = set()
    for name in found:
        forms.add(tuple(int(x) for x in re.search(r"ILi(\d+)ELi(\d+)ELi(\d+)EE", name).groups()))
    want = {(metric, d, e) for metric in (0, 1) for d in (128, 768) for e in (1, 2, 4)}
    assert want <= forms, sorted(want - forms)
    _check(found)
