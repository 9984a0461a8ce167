"""CPU test of the grouped BQ flow (wvg_search_group_bq_rescore / _bq_candidates,
wvg_group_bq.hip) from what can be read without a GPU: the built library's
gfx950 kernel descriptors (no private memory in the scan and the filter, the
rescore no more than rescore_keys_kernel's), the kernel names stay out of the
families tests/test_capi.py pins by pattern, and the Python and Go bindings
declare both entry points, Go checking its slice lengths before the cgo call."""
import os
import re
import subprocess

from test_capi import _gfx950_code_objects
from test_go_binding import go_source, strip_go_comments

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def _private_bytes(tmp_path):
    """{mangled kernel name: private_segment_fixed_size} of every gfx950 kernel in the library."""
    from weaviate_amd import _lib

    out = {}
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"gbq{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        name = None
        for ln in notes.splitlines():
            ln = ln.strip()
            if ln.startswith(".name:"):
                name = ln.split(":", 1)[1].strip()
            elif ln.startswith(".private_segment_fixed_size:") and name:
                out[name] = int(ln.split(":", 1)[1])
                name = None
    return out


def test_group_bq_kernels_private_segments(tmp_path):
    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain that built the library"
    priv = _private_bytes(tmp_path)
    scan = {int(m.group(1)): v for n, v in priv.items()
            for m in [re.search(r"\d+scan_bq_group_kernelILi(\d+)EE", n)] if m}
    assert set(scan) == {0, 1, 6, 12}, sorted(scan)  # K5's chunk counts: generic, d <= 128, 768, 1536
    assert not any(scan.values()), scan
    filt = [v for n, v in priv.items() if "bq_group_filter_kernel" in n]
    assert filt == [0], filt
    resc = {int(m.group(1)): v for n, v in priv.items()
            for m in [re.search(r"\d+rescore_group_kernelILi(\d+)EE", n)] if m}
    keys = {int(m.group(1)): v for n, v in priv.items()
            for m in [re.search(r"\d+rescore_keys_kernelILi(\d+)EE", n)] if m}
    assert set(resc) == set(keys) == {0, 1, 3, 4}, (sorted(resc), sorted(keys))
    for m in resc:
        assert resc[m] <= keys[m], (m, resc[m], keys[m])


def test_group_bq_kernel_names_stay_out_of_the_pinned_families(tmp_path):
    """tests/test_capi.py pins the K1 families and the hot kernels by name; the new kernels must
    not be counted among them (its hot list matches by substring)."""
    from test_capi import _k1_instantiations
    from weaviate_amd import _lib

    hot = ("scan_f32_stream_kernel", "scan_f32_kernel", "screen_ar_kernel", "screen_kernel", "scan_pq32_wide_kernel",
           "scan_pq32_rot_kernel", "scan_bq_kernel", "gemm_rs_kernel", "pq_encode_kernel", "merge_keys_kernel",
           "scan_f32_mq_kernel", "emit_prefix_kernel", "emit_filter_kernel", "emit_gather_kernel")
    new = [n for n in _private_bytes(tmp_path)
           if re.search(r"scan_bq_group_kernel|bq_group_filter_kernel|rescore_group_kernel", n)]
    assert len(new) == 9, new  # 4 scans, the filter, 4 metric kernels of the rescore
    for n in new:
        assert not any(h in n for h in hot), n
        assert not re.search(r"\d+(scan_f32_(?:stream_|mq_|qlist_)?kernel)I", n), n
    assert {f for f, _ in _k1_instantiations(_lib.LIB_PATH, tmp_path, READELF)} == {
        "scan_f32_kernel", "scan_f32_stream_kernel", "scan_f32_mq_kernel", "scan_f32_qlist_kernel"}


def test_python_binding_declares_both_entry_points():
    from weaviate_amd import _lib, device, flat

    assert len(_lib.SIGNATURES["wvg_search_group_bq_rescore"][1]) == 11
    assert len(_lib.SIGNATURES["wvg_search_group_bq_candidates"][1]) == 9
    assert callable(device.search_group_bq_rescore) and callable(device.search_group_bq_candidates)
    assert callable(flat.group_bq_kept_rows)
    lib = _lib.load()
    assert hasattr(lib, "wvg_search_group_bq_rescore") and hasattr(lib, "wvg_search_group_bq_candidates")
    assert _lib.ABI_VERSION == 3


def _go_func(src, signature):
    m = re.search(r"\nfunc " + signature + r"[^{]*\{", src)
    assert m, signature
    return src[m.end():src.index("\n}\n", m.end())]


def test_go_functions_check_lengths_before_the_call():
    src = strip_go_comments(go_source())
    body = _go_func(src, r"SearchGroupBQRescore\(bq, f32 \[\]\*Corpus, qs \[\]float32, k, rescoreLimit int, "
                         r"allows \[\]helpers\.AllowList\) \(\*Results, error\)")
    call = body.find("C.wvg_search_group_bq_rescore(")
    assert call > 0
    head = body[:call]
    assert re.search(r"len\(f32\) != len\(bq\) \{\s*return nil,", head)
    assert re.search(r"len\(qs\) != len\(bq\)\s*\*\s*[\w\[\]\.]+ \{\s*return nil,", head)
    assert re.search(r"len\(allows\) != 0 && len\(allows\) != len\(bq\) \{\s*return nil,", head)
    assert not re.search(r"IsEmpty\(\) \{\s*return", body)  # an empty list empties its own query only

    body = _go_func(src, r"SearchGroupBQCandidates\(bq \[\]\*Corpus, qs \[\]float32, rescoreLimit int, "
                         r"allows \[\]helpers\.AllowList\) \(\*Results, error\)")
    call = body.find("C.wvg_search_group_bq_candidates(")
    assert call > 0
    head = body[:call]
    assert re.search(r"len\(qs\) != len\(bq\)\s*\*\s*[\w\[\]\.]+ \{\s*return nil,", head)
    assert re.search(r"len\(allows\) != 0 && len\(allows\) != len\(bq\) \{\s*return nil,", head)
    assert not re.search(r"IsEmpty\(\) \{\s*return", body)
    # package-level functions, not methods
    assert not re.search(r"func \([^)]*\) SearchGroupBQ(Rescore|Candidates)\(", src)
    # the shared bitmap helper keeps a non-nil empty list a non-NULL pointer with zero words
    helper = _go_func(src, r"groupAllows\(allows \[\]helpers\.AllowList, nq int\)")
    assert re.search(r"if bitmaps\[i\] == nil \{\s*ap\[i\] = \(\*C\.uint64_t\)\(block\)", helper)
