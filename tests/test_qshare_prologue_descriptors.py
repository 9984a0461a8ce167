"""CPU test of the tile-parallel prologue (qshare_seed_kernel, qshare_seed_filt_kernel;
wvg_qshare.hip) from the built library's gfx950 kernel descriptors: all 24 forms
exist, none uses private memory, every one is built for the workgroup of
PRO_WAVES waves the launch uses and stays within the registers that shape
leaves a wave (a SIMD holds 512 VGPRs per lane: PRO_WAVES / 4 waves of a
workgroup share it) -- a whole 128-float tile row per lane is in flight, so the
forms at d = 128 hold at least those 128 -- and no name contains the substring
the bench and the traffic profile use to find the scan kernel."""
import os
import re
import subprocess

from test_capi import _gfx950_code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KEYS = (".private_segment_fixed_size", ".vgpr_count", ".agpr_count", ".max_flat_workgroup_size")


def _pro_waves():
    src = os.path.join(os.path.dirname(__file__), "..", "weaviate_amd", "csrc", "wvg_qshare.hip")
    return int(re.search(r"\bPRO_WAVES = (\d+);", open(src).read()).group(1))


def _prologue_kernels(tmp_path):
    """{(filtered, metric, D, E): {metadata key: value}} and the mangled names."""
    from weaviate_amd import _lib

    found, names = {}, []
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"qpro{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:  # a kernel's metadata block (its keys are sorted)
            block = ".agpr_count:" + block
            m = re.search(r"\.name:\s+(\S+)", block)
            if not m:
                continue
            n = re.search(r"\d+qshare_seed_(filt_)?kernelILi(\d+)ELi(\d+)ELi(\d+)EE", m.group(1))
            if not n:
                continue
            names.append(m.group(1))
            key = (n.group(1) is not None,) + tuple(int(x) for x in n.groups()[1:])
            found[key] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", block).group(1)) for k in KEYS}
    return found, names


def test_prologue_forms(tmp_path):
    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain that built the library"
    waves = _pro_waves()
    assert waves in (4, 8, 16)
    budget = 512 // (waves // 4)  # registers per lane a wave may hold with the workgroup resident on one CU
    found, names = _prologue_kernels(tmp_path)
    want = {(filt, metric, d, e) for filt in (False, True) for metric in (0, 1) for d in (128, 768) for e in (1, 2, 4)}
    assert want <= set(found), sorted(want - set(found))
    for key, md in found.items():
        assert md[".private_segment_fixed_size"] == 0, (key, md)
        assert md[".max_flat_workgroup_size"] == waves * 64, (key, md)
        assert md[".vgpr_count"] + md[".agpr_count"] <= min(budget, 512), (key, md)
        assert md[".agpr_count"] == 0, (key, md)
        if key[2] == 128:
            assert md[".vgpr_count"] >= 128, (key, md)  # the lane's whole row
    assert budget >= 256, "a whole tile in flight needs more than the 128 registers of 16 waves"
    assert not [n for n in names if "scan_f32_qshare" in n], names
