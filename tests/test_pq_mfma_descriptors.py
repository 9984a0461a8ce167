"""K8m's kernels (wvg_pq_mfma.hip) from the built library's gfx950 descriptors: each exists once and has no
private segment; the screen's static LDS is nothing beside the dynamic layout pq_mfma_supported sizes."""
import re
import subprocess

from test_capi import _gfx950_code_objects
from test_screen_l2_descriptors import READELF

KERNELS = ("pqm_screen_kernelILi4E", "pqm_screen_kernelILi8E", "pqm_prep_kernel", "pqm_norms_kernel",
           "pqm_qconst_kernel", "pqm_rescore_keys_kernel", "scan_pq_qlist_kernelILi4E")


def test_k8m_kernels_have_no_scratch(tmp_path):
    from weaviate_amd import _lib
    seen = set()
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"pm{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for item in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
            name = re.search(r"\.name:\s*(\S+)", item).group(1)
            for key in KERNELS:
                if key in name:
                    assert key not in seen, name
                    seen.add(key)
                    assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", item).group(1)) == 0, name
                    if "screen" in key:
                        assert int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", item).group(1)) == 0, name
    assert seen == set(KERNELS)
