"""K3c-W's kernels (wvg_screen.hip) from the built library's gfx950 descriptors: each exists once, has no
private segment, and its LDS -- dynamic, as launch_screen asks for it, + static -- fits a CU's 160 KB."""
import re
import subprocess

from test_capi import _gfx950_code_objects
from test_screen_l2_descriptors import LDS_LIMIT, READELF, SC_LDS_L2

# dynamic LDS launch_screen passes: K3c's SC_LDS for dot / cosine, + the workgroup's Cq for l2-squared
KERNELS = {
    "_ZN3wvg18screen_wide_kernelENS_14ScreenWideArgsE": SC_LDS_L2 - 128 * 4,
    "_ZN3wvg21screen_wide_l2_kernelENS_14ScreenWideArgsE": SC_LDS_L2,
    "screen_collect_wide_kernel": 0,
}


def test_wide_kernels_have_no_scratch_and_fit_lds(tmp_path):
    from weaviate_amd import _lib
    seen = {}
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"wd{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for item in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
            name = re.search(r"\.name:\s*(\S+)", item).group(1)
            for key, dyn in KERNELS.items():
                if key in name:
                    assert key not in seen, name
                    seen[key] = name
                    assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", item).group(1)) == 0, name
                    assert int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", item).group(1)) + dyn <= LDS_LIMIT
    assert set(seen) == set(KERNELS)
