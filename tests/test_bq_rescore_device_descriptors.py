"""CPU test of the fused device rescore (bq_rescore_kernel<METRIC, E, O512>, wvg_bq_rescore.hip) from the built
library's gfx950 kernel descriptors: it exists for both chain forms (L2, dot) x E in {1, 2, 4} x both distance
orders, none uses private memory or spills, and the two entry points are exported and bound.  What the kernel
computes: tests/test_gpu_bq_rescore_device.py."""
import ctypes
import re

from test_qshare_filter_descriptors import _kernels


def test_bq_rescore_kernels_and_entry_points(tmp_path):
    from weaviate_amd import _lib

    found = {}
    for name, d in _kernels(tmp_path, r"\d+bq_rescore_kernelILi\d+ELi\d+ELb[01]EE").items():
        key = tuple(int(g) for g in re.search(r"ILi(\d+)ELi(\d+)ELb([01])EE", name).groups())
        found[key] = (d[".private_segment_fixed_size"], d[".vgpr_spill_count"])
    want = {(metric, e, o512) for metric in (0, 1) for e in (1, 2, 4) for o512 in (0, 1)}
    assert set(found) == want, (sorted(want - set(found)), sorted(set(found) - want))
    assert set(found.values()) == {(0, 0)}, found
    for name in ("wvg_search_device_bq_rescore", "wvg_search_device_bq_rescore_workspace_size"):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and name in _lib.SIGNATURES, name
