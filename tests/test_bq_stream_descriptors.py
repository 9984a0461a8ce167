"""CPU test of the shared-row BQ scan (scan_bq_qshare_kernel<E, NCH, Q, FILT, PLAIN>,
wvg_bq_qshare.hip) from the built library's gfx950 kernel descriptors: it exists for every
E in {1, 2, 4} x NCH in {0, 1, 6, 12} x FILT x PLAIN at the one Q the host picks, none uses
private memory (8 lists indexed by anything but compile-time constants would), and none of
its names is mistaken for K5's by tests/test_capi.py's scan_bq_(group_)?kernel pattern.

The host functions behind the plan (queries per pass, row ranges) need a corpus, and a corpus
needs a device: tests/test_gpu_bq_stream.py::test_plan_and_errors pins them."""
import os
import re
import subprocess

from test_capi import _gfx950_code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
Q = 8  # bq_qshare_queries_per_pass


def _kernels(tmp_path):
    """({(E, NCH, Q, FILT, PLAIN): private_segment_fixed_size}, [kernel names]) of the library."""
    from weaviate_amd import _lib

    found, names = {}, []
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"bqs{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        key = None
        for ln in notes.splitlines():
            ln = ln.strip()
            if ln.startswith(".name:"):
                name = ln.split(":", 1)[1].strip()
                m = re.search(r"\d+scan_bq_qshare_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])EE", name)
                key = tuple(int(g) for g in m.groups()) if m else None
                if m:
                    names.append(name)
            elif ln.startswith(".private_segment_fixed_size:") and key:
                found[key] = int(ln.split(":", 1)[1])
                key = None
    return found, names


def test_bq_stream_kernels_exist_and_use_no_scratch(tmp_path):
    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain that built the library"
    found, names = _kernels(tmp_path)
    want = {(e, nch, Q, filt, plain) for e in (1, 2, 4) for nch in (0, 1, 6, 12) for filt in (0, 1) for plain in (0, 1)}
    assert set(found) == want, (sorted(want - set(found)), sorted(set(found) - want))
    spilled = {k: v for k, v in found.items() if v != 0}
    assert not spilled, spilled
    for name in names:  # K5's census (tests/test_capi.py) must not count these
        assert not re.search(r"\d+(scan_bq_(?:group_)?kernel)I((?:L[ib]\d+E)+)E", name), name
        assert "scan_bq_kernel" not in name, name
