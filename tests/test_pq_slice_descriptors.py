"""scan_pq_qshare_slice_kernel<E, 4, FILT, PLAIN> (wvg_pq_qslice.hip) in the built library's gfx950 kernel
descriptors: every E x FILT x PLAIN exists, with no private memory, at most the 128 VGPRs a lane of a
1024-thread workgroup has and 8 KiB x E of static LDS; scan_pq_qshare_kernel keeps what
test_pq_stream_descriptors.py expects of it."""
import re
import subprocess

from test_capi import _gfx950_code_objects
from test_pq_stream_descriptors import FORMS, READELF, _kernels


def test_pq_slice_kernels(tmp_path):
    from weaviate_amd import _lib

    found, cur = {}, {}
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"pqsl{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for ln in notes.splitlines():  # a kernel's fields in alphabetical order, .agpr_count .. .wavefront_size
            field, _, value = ln.strip().lstrip("- ").partition(":")
            cur[field] = value.strip()
            if field == ".wavefront_size":
                m = re.search(r"\d+scan_pq_qshare_slice_kernelILi(\d+)ELi4ELb([01])ELb([01])EE", cur.get(".name", ""))
                if m:
                    found[tuple(int(g) for g in m.groups())] = cur
                cur = {}
    assert set(found) == {(e, filt, plain) for e in (1, 2, 4) for filt in (0, 1) for plain in (0, 1)}
    for (e, _, _), d in found.items():
        assert int(d[".private_segment_fixed_size"]) == 0 and int(d[".group_segment_fixed_size"]) == 8192 * e, d
        assert int(d[".vgpr_count"]) + int(d[".agpr_count"]) <= 128, d
    whole, _ = _kernels(tmp_path)
    assert len(whole) == 12 * len(FORMS) and not any(whole.values()), whole
