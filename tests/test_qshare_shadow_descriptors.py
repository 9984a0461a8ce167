"""CPU test of the shadow-fed screened shared-row scan (scan_f32_qshare_shadow_kernel and its
filtered twin; wvg_qshare.hip) from the built library's gfx950 kernel descriptors: each exists
exactly once, uses no private memory and stays within the 256 registers of the two waves per SIMD
it is built for (amdgpu_waves_per_eu(2, 2)); the prologue, whose query side gained a second branch
(QShareArgs::screen = 2), keeps its three L2 instantiations without private memory within 256."""
import os

from test_qshare_screen_descriptors import READELF, _kernels

WAVES_PER_EU = 2
REG_LIMIT = 512 // WAVES_PER_EU  # a SIMD's 512 registers per lane, shared by its waves


def test_shadow_scan_kernels_exist_once_without_scratch(tmp_path):
    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain that built the library"
    plain = _kernels(tmp_path, r"\d+scan_f32_qshare_shadow_kernelE")
    filt = _kernels(tmp_path, r"\d+scan_f32_qshare_shadow_filt_kernelE")
    assert len(plain) == 1, sorted(plain)
    assert len(filt) == 1, sorted(filt)
    for name, md in {**plain, **filt}.items():
        print(name, md)
        assert md[".private_segment_fixed_size"] == 0, (name, md)
        assert md[".vgpr_count"] <= REG_LIMIT and md[".agpr_count"] <= md[".vgpr_count"], (name, md)


def test_prologue_keeps_its_instantiations_without_scratch(tmp_path):
    seed = _kernels(tmp_path, r"\d+qshare_seed_kernelILi0ELi128ELi[124]EE")
    assert len(seed) == 3, sorted(seed)
    for name, md in seed.items():
        print(name, md)
        assert md[".private_segment_fixed_size"] == 0, (name, md)
        assert md[".vgpr_count"] <= 256 and md[".agpr_count"] <= md[".vgpr_count"], (name, md)
