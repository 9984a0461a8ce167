"""CPU test of the shared-row PQ scan (scan_pq_qshare_kernel<E, ROT, Q, FILT, PLAIN>,
wvg_pq_qshare.hip) from the built library's gfx950 kernel descriptors: it exists for every
E in {1, 2, 4} x form x Q the host can pick for that form (the rotated m = 32, ks = 256 form
has 16-byte image entries, Q = 4; the generic form runs at Q = 4 and Q = 2) x FILT x PLAIN,
none uses private memory (Q lists indexed by anything but compile-time constants would), and
none of its names is mistaken for K8 / K8b / K8e by the censuses of the existing tests.

The host functions behind the plan (queries per pass, row ranges) need a corpus, and a corpus
needs a device: tests/test_gpu_pq_stream.py::test_plan_and_errors pins them."""
import os
import re
import subprocess

from test_capi import _gfx950_code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
FORMS = [(1, 4), (0, 4), (0, 2)]  # (ROT, Q)


def _kernels(tmp_path):
    """({(E, ROT, Q, FILT, PLAIN): private_segment_fixed_size}, [kernel names]) of the library."""
    from weaviate_amd import _lib

    found, names = {}, []
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"pqs{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        key = None
        for ln in notes.splitlines():
            ln = ln.strip()
            if ln.startswith(".name:"):
                name = ln.split(":", 1)[1].strip()
                m = re.search(r"\d+scan_pq_qshare_kernelILi(\d+)ELb([01])ELi(\d+)ELb([01])ELb([01])EE", name)
                key = tuple(int(g) for g in m.groups()) if m else None
                if m:
                    names.append(name)
            elif ln.startswith(".private_segment_fixed_size:") and key:
                found[key] = int(ln.split(":", 1)[1])
                key = None
    return found, names


def test_pq_stream_kernels_exist_and_use_no_scratch(tmp_path):
    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain that built the library"
    found, names = _kernels(tmp_path)
    want = {(e, rot, q, filt, plain) for e in (1, 2, 4) for rot, q in FORMS for filt in (0, 1) for plain in (0, 1)}
    assert set(found) == want, (sorted(want - set(found)), sorted(set(found) - want))
    spilled = {k: v for k, v in found.items() if v != 0}
    assert not spilled, spilled
    for name in names:  # the K8 / K8b / K8e censuses must not count these
        for other in ("scan_pq32_wide_kernel", "scan_pq32_rot_kernel", "scan_pq_kernel"):
            assert other not in name, name
