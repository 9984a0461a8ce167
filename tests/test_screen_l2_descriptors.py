"""CPU test of K3c-L2 (screen_l2_kernel, wvg_screen.hip) from the built library's
gfx950 kernel descriptors: the kernel exists once, has no private segment, its
LDS fits, its register counts are the ones DESIGN.md states -- and the eight
dot / cosine screen kernels (every kernel that takes a ScreenArgs) keep the
VGPR count, static LDS size and private segment they had before K3c-L2 shared
K3c's body (read from a build of the parent commit)."""
import os
import re
import subprocess

from test_capi import _gfx950_code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("vgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size")

# (vgpr_count, group_segment_fixed_size, private_segment_fixed_size) on the parent commit
PARENT = {
    "_ZN3wvg13screen_kernelENS_10ScreenArgsE": (146, 0, 0),
    "_ZN3wvg16screen_ar_kernelILi16ELi0ELb0EEEvNS_10ScreenArgsE": (412, 0, 0),
    "_ZN3wvg16screen_ar_kernelILi24ELi0ELb0EEEvNS_10ScreenArgsE": (500, 0, 0),
    "_ZN3wvg16screen_ar_kernelILi8ELi0ELb1EEEvNS_10ScreenArgsE": (380, 0, 0),
    "_ZN3wvg16screen_ar_kernelILi12ELi0ELb1EEEvNS_10ScreenArgsE": (396, 0, 0),
    "_ZN3wvg16screen_ar_kernelILi16ELi0ELb1EEEvNS_10ScreenArgsE": (456, 0, 0),
    "_ZN3wvg16screen_i8_kernelILi8ELi0EEEvNS_10ScreenArgsE": (384, 0, 0),
    "_ZN3wvg16screen_i8_kernelILi12ELi0EEEvNS_10ScreenArgsE": (484, 0, 0),
}
LDS_LIMIT = 163_840
# K3c's dynamic LDS (SC_LDS: four stages of 8 + 16 + 1 KiB and 256 B, the wave lists, the thresholds, three
# per-query constants) + the workgroup's Cq
SC_LDS_L2 = 4 * (25 * 1024 + 256) + 8 * 32 * 16 * 8 + 8 * 32 * 4 * 2 + 128 * 4 * 3 + 128 * 4


def _descriptors(tmp_path):
    """{mangled name: {key: value}} of every gfx950 kernel whose name mentions a screen argument struct."""
    from weaviate_amd import _lib

    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain that built the library"
    out = []
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"l2d{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for item in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
            item = ".agpr_count:" + item
            m = re.search(r"\.name:\s*(\S+)", item)
            if not m or not re.search(r"\d+Screen(L2)?ArgsE", m.group(1)):
                continue
            d = {k: int(re.search(r"\." + k + r":\s*(\d+)", item).group(1)) for k in KEYS}
            out.append((m.group(1), d))
    return out


def test_l2_kernel_descriptor_matches_design(tmp_path):
    l2 = [d for n, d in _descriptors(tmp_path) if n == "_ZN3wvg16screen_l2_kernelENS_12ScreenL2ArgsE"]
    assert len(l2) == 1, l2
    d = l2[0]
    assert d["private_segment_fixed_size"] == 0
    assert d["group_segment_fixed_size"] + SC_LDS_L2 <= LDS_LIMIT
    src = open(os.path.join(ROOT, "weaviate_amd", "csrc", "wvg_screen.hip")).read()
    assert "constexpr int SC_LDS_L2 = SC_LDS + SC_BQ * 4;" in src  # the dynamic LDS launch_screen asks for
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"screen_l2_kernel`?: (\d+) VGPRs, (\d+) AGPRs, ([\d,]+) B of LDS", design)
    assert m, "DESIGN.md states K3c-L2's descriptor"
    assert (d["vgpr_count"], d["agpr_count"]) == (int(m.group(1)), int(m.group(2)))
    assert int(m.group(3).replace(",", "")) == SC_LDS_L2 + d["group_segment_fixed_size"]


def test_dot_cosine_screen_kernels_keep_their_descriptors(tmp_path):
    got = {n: (d["vgpr_count"], d["group_segment_fixed_size"], d["private_segment_fixed_size"])
           for n, d in _descriptors(tmp_path) if "10ScreenArgsE" in n}
    assert got == PARENT
    # and no other kernel takes the L2 argument struct
    assert [n for n, _ in _descriptors(tmp_path) if "12ScreenL2ArgsE" in n] == [
        "_ZN3wvg16screen_l2_kernelENS_12ScreenL2ArgsE"]
