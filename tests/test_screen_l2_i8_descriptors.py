"""CPU test of the K3i-L2 kernels (wvg_screen.hip) from the built library's gfx950 kernel descriptors: the
three kernels exist once each, use no scratch, and their LDS (dynamic, as launch_screen asks for it, + static)
fits the 160 KiB of a CU."""
import os
import re
import subprocess

from test_capi import _gfx950_code_objects
from test_screen_l2_descriptors import LDS_LIMIT, READELF

SJ_LDS_L2 = 7 * 16384 + 2 * 2304 + 4 * 64 * 16 * 8 + 4 * 64 * 4 * 2 + 128 * 4 * 6  # 2 x 2: 7 stages, Cq
SI_LDS_L2 = 8 * 16384 + 2 * 2304 + 4 * 32 * 16 * 8 + 4 * 32 * 4 * 2 + 128 * 4 * 6  # 1 x 4: 8 stages, Cq
WANT = {"_ZN3wvg19screen_i8_l2_kernelILi8EEEvNS_14ScreenL2I8ArgsE": SJ_LDS_L2,
        "_ZN3wvg19screen_i8_l2_kernelILi12EEEvNS_14ScreenL2I8ArgsE": SJ_LDS_L2,
        "_ZN3wvg19screen_ar_l2_kernelILi16EEEvNS_14ScreenL2I8ArgsE": SI_LDS_L2}


def test_l2_i8_kernels_exist_without_scratch(tmp_path):
    from weaviate_amd import _lib

    assert os.path.exists(READELF)
    got = {}
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"l2i8d{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for item in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
            m = re.search(r"\.name:\s*(\S+)", item)
            if m and "14ScreenL2I8ArgsE" in m.group(1):
                assert m.group(1) not in got
                got[m.group(1)] = {k: int(re.search(r"\." + k + r":\s*(\d+)", item).group(1))
                                   for k in ("group_segment_fixed_size", "private_segment_fixed_size")}
    assert sorted(got) == sorted(WANT)
    for name, d in got.items():
        assert d["private_segment_fixed_size"] == 0, name
        assert d["group_segment_fixed_size"] + WANT[name] <= LDS_LIMIT, name
