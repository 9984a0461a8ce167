"""K8m-S's screen kernels (wvg_pq_mfma.hip) from the built library's gfx950 descriptors: each instantiation exists
once, has no private segment and no static LDS beside its dynamic layout."""
import re
import subprocess

from test_capi import _gfx950_code_objects
from test_screen_l2_descriptors import READELF

KERNELS = ("pqs_screen_kernelILi4ELb0E", "pqs_screen_kernelILi8ELb0E", "pqs_screen_kernelILi8ELb1E")


def test_k8ms_kernels_have_no_scratch(tmp_path):
    from weaviate_amd import _lib
    seen = []
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"ps{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for item in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
            name = re.search(r"\.name:\s*(\S+)", item).group(1)
            if "pqs_screen_kernel" in name:
                seen.append(next((key for key in KERNELS if key in name), name))
                for seg in ("private", "group"):
                    assert int(re.search(rf"\.{seg}_segment_fixed_size:\s*(\d+)", item).group(1)) == 0, name
    assert sorted(seen) == sorted(KERNELS)
