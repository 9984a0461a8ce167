"""CPU test of the grouped-search kernels (scan_f32_group_kernel /
merge_group_kernel, wvg_group.hip) from the built library's gfx950 kernel
descriptors: no instantiation uses private memory ("A
scratch regression and its guard"), the compiled (metric, D, E) forms are
exactly those tests/test_gpu_group.py runs, and the Go binding's SearchGroup
checks its slice lengths before the call."""
import os
import re
import subprocess

from test_capi import _gfx950_code_objects
from test_go_binding import go_source, strip_go_comments

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def _group_kernels(tmp_path):
    """({(metric, D, E): private bytes} of scan_f32_group_kernel, {E: private bytes} of merge_group_kernel)."""
    from weaviate_amd import _lib

    scan, merge = {}, {}
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"grp{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        name = None
        for ln in notes.splitlines():
            ln = ln.strip()
            if ln.startswith(".name:"):
                name = None
                m = re.search(r"\d+scan_f32_group_kernelILi(\d+)ELi(\d+)ELi(\d+)EE", ln)
                if m:
                    name = (scan, tuple(int(x) for x in m.groups()))
                m = re.search(r"\d+merge_group_kernelILi(\d+)EE", ln)
                if m:
                    name = (merge, int(m.group(1)))
            elif ln.startswith(".private_segment_fixed_size:") and name:
                name[0][name[1]] = int(ln.split(":", 1)[1])
                name = None
    return scan, merge


def test_group_kernels_use_no_scratch_and_match_the_gpu_matrix(tmp_path):
    from test_gpu_group import GROUP, kernel_forms

    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain that built the library"
    scan, merge = _group_kernels(tmp_path)
    assert scan and merge, "the library holds no grouped-search kernels"
    spilled = {k: v for k, v in {**scan, **{("merge", e): v for e, v in merge.items()}}.items() if v != 0}
    assert not spilled, spilled
    # K1's matrix: the four metric kernels x {128, 768, 1536, generic} x E in {1, 2, 4}
    want = {(m, d, e) for m in (0, 1, 3, 4) for d in GROUP["fixed_d"] + (0,) for e in (1, 2, 4)}
    assert set(scan) == want, sorted(set(scan) ^ want)
    assert set(scan) == kernel_forms(), sorted(set(scan) ^ kernel_forms())  # every compiled form is run on the GPU
    assert set(merge) == {1, 2, 4}


def test_group_kernel_names_stay_out_of_the_k1_families(tmp_path):
    """tests/test_capi.py pins the K1 families by name pattern; the grouped kernels must not match it."""
    from test_capi import _k1_instantiations
    from weaviate_amd import _lib

    assert not re.search(r"\d+(scan_f32_(?:stream_|mq_|qlist_)?kernel)I", "21scan_f32_group_kernelILi0ELi128ELi1EE")
    assert {f for f, _ in _k1_instantiations(_lib.LIB_PATH, tmp_path, READELF)} == {
        "scan_f32_kernel", "scan_f32_stream_kernel", "scan_f32_mq_kernel", "scan_f32_qlist_kernel"}


def test_go_search_group_checks_lengths_before_the_call():
    src = strip_go_comments(go_source())
    m = re.search(r"\nfunc SearchGroup\(corpora \[\]\*Corpus, qs \[\]float32, k int, allows \[\]helpers\.AllowList\)"
                  r"[^{]*\{", src)
    assert m, "package-level func SearchGroup(corpora []*Corpus, qs []float32, k int, allows []helpers.AllowList)"
    body = src[m.end():src.index("\n}\n", m.end())]
    call = body.find("C.wvg_search_group(")
    assert call > 0
    head = body[:call]
    assert re.search(r"len\(qs\) != len\(corpora\)\s*\*\s*\w+ \{\s*return nil,", head)
    assert re.search(r"len\(allows\) != 0 && len\(allows\) != len\(corpora\) \{\s*return nil,", head)
    # one list per query: a non-nil empty list must not end the call for the other queries
    assert not re.search(r"IsEmpty\(\) \{\s*return", body)
    assert not re.search(r"func \([^)]*\) SearchGroup\(", src)


def test_python_binding_declares_the_entry_point():
    from weaviate_amd import _lib, device, flat

    assert len(_lib.SIGNATURES["wvg_search_group"][1]) == 9
    assert callable(device.search_group) and callable(flat.SearchByVectorGroup)
    assert hasattr(_lib.load(), "wvg_search_group")
