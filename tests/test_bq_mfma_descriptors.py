"""K5m's kernels (wvg_bq_mfma.hip) from the built library's gfx950 descriptors: both query-block forms exist
once, have no private segment, and their LDS -- the largest image launch_bq_mfma stages (128 KiB) plus the
bounds, counts, thresholds and flags behind it, + static -- fits a CU's 160 KB."""
import re
import subprocess

from test_capi import _gfx950_code_objects
from test_screen_l2_descriptors import LDS_LIMIT, READELF

DYNAMIC = 128 * 1024 + 64 * 8 + 64 * 4 + 64 * 4 + 16
KERNELS = ("scan_bq_mfma_kernelILi4E", "scan_bq_mfma_kernelILi2E", "bqm_image_kernel")


def test_k5m_kernels_have_no_scratch_and_fit_lds(tmp_path):
    from weaviate_amd import _lib
    seen = set()
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"bm{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for item in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
            name = re.search(r"\.name:\s*(\S+)", item).group(1)
            for key in KERNELS:
                if key in name:
                    assert key not in seen, name
                    seen.add(key)
                    assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", item).group(1)) == 0, name
                    dyn = DYNAMIC if "scan" in key else 0
                    assert int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", item).group(1)) + dyn <= LDS_LIMIT
    assert seen == set(KERNELS)
