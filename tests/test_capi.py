"""CPU tests of the C-ABI library: it loads and exports every symbol the
public header declares; calls that need a device fail with a status code
(never abort) when there is none."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wvgpu.h")


def header_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(wvg_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_header_symbol():
    from weaviate_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = header_symbols()
    assert len(syms) >= 25
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing


def test_binding_covers_header():
    from weaviate_amd import _lib

    assert set(header_symbols()) == set(_lib.SIGNATURES)


def test_abi_version_and_error_path():
    from weaviate_amd import _lib

    lib = _lib.load()
    assert lib.wvg_abi_version() == _lib.ABI_VERSION == 3
    # a null-argument call returns a negative status and sets the message
    rc = lib.wvg_device_count(None)
    assert rc == _lib.WVG_ERR_INVALID
    assert b"null" in lib.wvg_last_error()


def test_library_is_gfx950_code_object():
    from weaviate_amd import _lib

    data = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in data


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_open_without_device_fails_cleanly():
    from weaviate_amd import _lib

    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.wvg_open(0, ctypes.byref(h))
    assert rc in (_lib.WVG_ERR_DEVICE, _lib.WVG_ERR_INVALID)
    assert not h.value


def test_exports_equal_header():
    """The product library exports exactly the header's entry points: no
    tuning setter (wvgx_*), no A/B knobs -- those live in the tools build."""
    import subprocess

    from weaviate_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("wvg")}
    assert exported == set(header_symbols())


def test_options_struct_matches_library():
    import ctypes as ct

    from weaviate_amd import _lib

    lib = _lib.load()
    o = _lib.Options()
    lib.wvg_options_default(ct.byref(o))
    assert o.size == ct.sizeof(_lib.Options)
    assert (o.mfma_min_queries, o.cache_reuse, o.merge_wait_us, o.batch_screen, o.coalesce) == (32, 1, 0, 2, 1)
    bad = _lib.Options()
    lib.wvg_options_default(ct.byref(bad))
    bad.size = 3
    h = ct.c_void_p()
    assert lib.wvg_open_ex(0, ct.byref(bad), ct.byref(h)) == _lib.WVG_ERR_INVALID
    assert not h.value


def _gfx950_code_objects(path):
    """The gfx950 code objects of the library's offload bundles (one per translation unit)."""
    import struct

    data = open(path, "rb").read()
    out, i = [], data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    while i >= 0:
        n = struct.unpack_from("<Q", data, i + 24)[0]
        p = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            p += 24
            triple = data[p:p + tl]
            p += tl
            if b"gfx950" in triple and size:
                out.append(data[i + off:i + off + size])
        i = data.find(b"__CLANG_OFFLOAD_BUNDLE__", i + 24)
    return out


def test_hot_kernels_use_no_scratch(tmp_path):
    """No hot-path kernel spills or copies its arguments to scratch: round 5 once
    regressed the query-stream scan from 83 to 150 us per 1M-row query when an
    un-inlined lambda forced the kernel arguments (the inline query) into
    private memory.  Checked from the code objects' metadata."""
    import subprocess

    from weaviate_amd import _lib

    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    hot = ("scan_f32_stream_kernel", "scan_f32_kernel", "screen_ar_kernel", "screen_i8_kernel", "screen_kernel",
           "scan_pq32_wide_kernel", "scan_pq32_rot_kernel", "scan_bq_kernel", "gemm_rs_kernel", "pq_encode_kernel",
           "merge_keys_kernel", "scan_f32_mq_kernel", "emit_prefix_kernel", "emit_filter_kernel", "emit_gather_kernel")
    bad, seen = [], 0
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"co{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([readelf, "--notes", str(f)], capture_output=True, text=True).stdout
        name = None
        for ln in notes.splitlines():
            ln = ln.strip()
            if ln.startswith(".name:"):
                name = ln.split(":", 1)[1].strip()
            elif ln.startswith(".private_segment_fixed_size:") and name and any(h in name for h in hot):
                seen += 1
                if int(ln.split(":", 1)[1]) != 0:
                    bad.append(name)
    # known: K3b at d = 512 with two waves per SIMD (256 registers) spills one VGPR (8 bytes); it is the
    # exact fallback of d = 512 batches (k > 16 or batch_screen = 0), not the screen's path
    known = ("gemm_rs_kernelILi512ELi1ELi2ELi2E",)
    bad = [n for n in bad if not any(k in n for k in known)]
    assert seen > 20, seen
    assert not bad, bad


K1_FAMILIES = ("scan_f32_kernel", "scan_f32_stream_kernel", "scan_f32_mq_kernel", "scan_f32_qlist_kernel")


def _k1_instantiations(lib_path, tmp_path, readelf):
    """{(family, (metric, D, E, ...))} of the K1 kernels in the library's gfx950 code
    objects, parsed from the mangled kernel names (...kernelILi<metric>ELi<D>ELi<E>E...)."""
    import subprocess

    found = set()
    for j, co in enumerate(_gfx950_code_objects(lib_path)):
        f = tmp_path / f"k1co{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([readelf, "--notes", str(f)], capture_output=True, text=True).stdout
        for ln in notes.splitlines():
            ln = ln.strip()
            if not ln.startswith(".name:"):
                continue
            m = re.search(r"\d+(scan_f32_(?:stream_|mq_|qlist_)?kernel)I((?:L[ib]\d+E)+)E", ln)
            if m:
                found.add((m.group(1), tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(2)))))
    return found


def test_k1_matrix_covers_every_specialization(tmp_path):
    """The fixed row lengths and register-list sizes the K1 kernels are compiled for are
    exactly those tests/test_gpu_k1_matrix.py runs against the oracle: a new `case <D>:`
    of the scan dispatch fails here until the matrix has a row for it.  The last loop
    also pins that every family is built for every metric kernel and list size: pruning
    instantiations (e.g. the scan_f32_qlist_kernel forms without a caller,
    profiles/r07/k1_matrix/README.md) means updating it."""
    from test_gpu_k1_matrix import DIMS, K1
    from weaviate_amd import _lib

    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    found = _k1_instantiations(_lib.LIB_PATH, tmp_path, readelf)
    assert {f for f, _ in found} == set(K1_FAMILIES)
    fixed = set(K1["fixed_d"])
    assert fixed <= set(DIMS) and any(d not in fixed for d in DIMS)  # every fixed length and a generic one are run
    assert {a[1] for _, a in found} == fixed | {0}
    for fam in ("scan_f32_kernel", "scan_f32_stream_kernel"):
        assert {a[1] for f, a in found if f == fam} == fixed | {0}, fam
    assert {a[2] for _, a in found} == set(K1["e"]) == {1, 2, 4}
    assert {a[1] for f, a in found if f == "scan_f32_mq_kernel"} == set(K1["mq_d"]) == {128, 768}
    for fam in K1_FAMILIES:  # every family in every list size and metric kernel (K1Q: L2 / dot only)
        assert {a[0] for f, a in found if f == fam} == ({0, 1} if fam == "scan_f32_mq_kernel" else {0, 1, 3, 4}), fam
        assert {a[2] for f, a in found if f == fam} == {1, 2, 4}, fam


def _k5_instantiations(lib_path, tmp_path, readelf):
    """{(kernel, (template arguments...))} of scan_bq_kernel<E, NCH, COS, EMIT> and
    scan_bq_group_kernel<NCH> in the library's gfx950 code objects, parsed from the mangled
    kernel names (...scan_bq_kernelILi<E>ELi<NCH>ELb<COS>ELi<EMIT>EE...)."""
    import subprocess

    found = set()
    for j, co in enumerate(_gfx950_code_objects(lib_path)):
        f = tmp_path / f"k5co{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([readelf, "--notes", str(f)], capture_output=True, text=True).stdout
        for ln in notes.splitlines():
            ln = ln.strip()
            if not ln.startswith(".name:"):
                continue
            m = re.search(r"\d+(scan_bq_(?:group_)?kernel)I((?:L[ib]\d+E)+)E", ln)
            if m:
                found.add((m.group(1), tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(2)))))
    return found


def test_k5_matrix_covers_every_specialization(tmp_path):
    """The chunk counts, list sizes and record modes scan_bq_kernel is compiled for are exactly
    those tests/test_gpu_bq_k5_matrix.py runs against the oracle, each fixed chunk count with an
    even and an odd word count: a new `case N:` of launch_bq_ec (or of the group kernel's
    dispatch) fails here until the matrix has rows for it."""
    import itertools

    from test_gpu_bq_k5_matrix import DIMS, K5, nch_of, words_of
    from weaviate_amd import _lib

    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    found = _k5_instantiations(_lib.LIB_PATH, tmp_path, readelf)
    assert K5 == {"nch": (1, 6, 12), "e": (1, 2, 4), "emit": (0, 1, 2)}
    nchs = set(K5["nch"]) | {0}
    scan = {a for f, a in found if f == "scan_bq_kernel"}
    assert scan == set(itertools.product(K5["e"], nchs, (0, 1), K5["emit"])), sorted(scan)
    assert len(scan) == 72
    assert {a for f, a in found if f == "scan_bq_group_kernel"} == {(n,) for n in nchs}
    for nch in K5["nch"]:  # every fixed chunk count runs with an even and with an odd word count
        assert {words_of(d) % 2 for d in DIMS if nch_of(d) == nch} == {0, 1}, nch
    assert any(nch_of(d) == 0 for d in DIMS)  # and the generic loop


def _screen_instantiations(lib_path, tmp_path, readelf):
    """{(kernel, (template arguments...))} of the batched screen's scoring kernels -- every
    kernel that takes a ScreenArgs -- in the library's gfx950 code objects, parsed from the
    mangled names (screen_kernel, screen_ar_kernelILi<KBN>ELi<DIAG>ELb<I8>EE, ...)."""
    import subprocess

    found = set()
    for j, co in enumerate(_gfx950_code_objects(lib_path)):
        f = tmp_path / f"scco{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([readelf, "--notes", str(f)], capture_output=True, text=True).stdout
        for ln in notes.splitlines():
            ln = ln.strip()
            if not ln.startswith(".name:") or "10ScreenArgs" not in ln:
                continue
            m = re.search(r"\d+(screen\w*_kernel)(?:I((?:L[ib]\d+E)+)E)?", ln)
            assert m, ln
            found.add((m.group(1), tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(2) or ""))))
    return found


def test_product_screen_kernels_are_the_pinned_set(tmp_path):
    """The product library holds exactly the eight screen kernels launch_screen's table
    names: K3c, K3d <KBN, DIAG, I8> for 16 / 24 bf16 and 8 / 12 / 16 int8 K blocks, K3i
    2 x 2 <KBN, DIAG> for 8 / 12 -- no diagnostic (DIAG != 0) and no retired variant.
    A new instantiation fails here until tests/test_gpu_screen.py covers it."""
    from weaviate_amd import _lib

    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    found = _screen_instantiations(_lib.LIB_PATH, tmp_path, readelf)
    assert found == {
        ("screen_kernel", ()),
        ("screen_ar_kernel", (16, 0, 0)), ("screen_ar_kernel", (24, 0, 0)),
        ("screen_ar_kernel", (8, 0, 1)), ("screen_ar_kernel", (12, 0, 1)), ("screen_ar_kernel", (16, 0, 1)),
        ("screen_i8_kernel", (8, 0)), ("screen_i8_kernel", (12, 0)),
    }, sorted(found)
