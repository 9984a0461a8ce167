"""CPU test of the device select route (wvg_dselect.hip: wvg_search_device with k > 256) from the
built library's gfx950 kernel descriptors: every kernel of the route exists -- the shared-row keys
kernel for both raw sums (l2-squared; dot, which cosine shares) at 4 queries per group, the select
(init, histogram, pick), the rank, scan and compaction kernels and the emit kernel -- none uses
private memory (the keys kernel holds 4 queries' 4 x 8 accumulators in registers; an accumulator
set indexed by anything but compile-time constants, or a fifth query, would spill), and none of
their names is mistaken for another kernel family by the censuses of the existing tests."""
import os
import re
import subprocess

from test_capi import _gfx950_code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
WVG_M_L2, WVG_M_DOT = 0, 1
PLAIN = ["dsel_init_kernel", "dsel_hist_kernel", "dsel_pick_kernel", "dsel_rank_kernel", "dsel_scan_kernel",
         "dsel_compact_kernel", "dsel_emit_kernel"]
FAMILIES = ["scan_f32_kernel", "scan_f32_stream_kernel", "scan_f32_mq_kernel", "screen_kernel", "screen_ar_kernel",
            "screen_i8_kernel", "merge_keys_kernel", "emit_prefix_kernel", "emit_filter_kernel", "emit_gather_kernel",
            "scan_bq_kernel", "scan_pq_kernel", "scan_pq32_", "gemm_rs_kernel", "pq_encode_kernel"]


def _kernels(tmp_path):
    """{kernel key: private_segment_fixed_size} and the mangled names of the dsel_ kernels; a key is the
    plain kernel's name or ("dsel_keys_f32_kernel", METRIC, G)."""
    from weaviate_amd import _lib

    found, names = {}, []
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"dsel{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        key = None
        for ln in notes.splitlines():
            ln = ln.strip()
            if ln.startswith(".name:"):
                name = ln.split(":", 1)[1].strip()
                key = None
                m = re.search(r"\d+dsel_keys_f32_kernelILi(\d+)ELi(\d+)EE", name)
                if m:
                    key = ("dsel_keys_f32_kernel", int(m.group(1)), int(m.group(2)))
                else:
                    m = re.search(r"\d+(dsel_[a-z0-9_]+_kernel)E", name)
                    key = m.group(1) if m else None
                if key:
                    names.append(name)
            elif ln.startswith(".private_segment_fixed_size:") and key:
                found[key] = int(ln.split(":", 1)[1])
                key = None
    return found, names


def test_device_select_kernels_exist_and_use_no_scratch(tmp_path):
    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain that built the library"
    found, names = _kernels(tmp_path)
    want = set(PLAIN) | {("dsel_keys_f32_kernel", m, 4) for m in (WVG_M_L2, WVG_M_DOT)}
    assert set(found) == want, (sorted(map(str, want - set(found))), sorted(map(str, set(found) - want)))
    spilled = {k: v for k, v in found.items() if v != 0}
    assert not spilled, spilled
    for name in names:
        for other in FAMILIES:
            assert other not in name, name
