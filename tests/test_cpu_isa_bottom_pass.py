"""Cache policy of the CFFT tile accesses in the built code object (CPU-only, beside test_cpu_isa.py: the gfx950 code object is
taken out of the in-tree cfft.o; nothing is executed).  DESIGN.md 4.1: the forward pass kernels that cfft.hip launches for column
sets far larger than the cache (k_cfft_b_stream, k_cfft_a_stream) carry the non-temporal policy on every tile load and store --
loads AND stores, since the in-place read-modify-write loses with either alone (tools/microbench7.hip) -- and not on the twiddle
loads, which every column of a tile position shares; the kernels every other transform runs on carry it nowhere.  The forward
2^13 bottom pass keeps its resources in both forms: no scratch, and LDS such that three workgroups share a CU's 160 KiB."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "tstwo_amd", "csrc", "obj", "cfft.o")
LLVM = "/opt/rocm/lib/llvm/bin"
BOTTOM, BOTTOM_STREAM = r"k_cfft_bILb0ELi13ELb0E", r"k_cfft_b_streamILi13E"
STRIDED, STRIDED_STREAM = r"k_cfft_aILb0ELi9ELi0ELi15E", r"k_cfft_a_streamILi9E"
LOGT = 13
DYNAMIC_LDS = ((1 << LOGT) + (1 << (LOGT - 5)) + (1 << (LOGT - 4))) * 4      # padded tile + twiddle heap (cfft_plan.h: cfft_plan)
CU_LDS = 160 * 1024


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    if not os.path.exists(OBJ):
        pytest.skip("library objects not built (python -m tstwo_amd.build)")
    if not (shutil.which("objcopy") and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("binutils / ROCm LLVM tools not available")
    d = tmp_path_factory.mktemp("bottom_pass")
    fat, co = str(d / "fat.bin"), str(d / "dev.co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", OBJ, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co])
    return co


def _metadata(co, kernel):
    """{field: int} of the kernel's entry in the code object's metadata note."""
    text = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    entries = [e for e in re.split(r"\n\s*- \.agpr_count:", text) if re.search(r"\.name:\s+\S*" + kernel, e)]
    assert len(entries) == 1, len(entries)
    return {k: int(v) for k, v in re.findall(r"\.(vgpr_count|private_segment_fixed_size|group_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)", entries[0])}


def _memory_instructions(co, kernel):
    """The global loads and stores of the one kernel whose name matches."""
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
    found, inside, out = 0, False, []
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            inside = bool(re.search(kernel, m.group(1)))
            found += inside
        elif inside:
            ins = line.split("//")[0].strip()
            if ins.startswith(("global_load", "global_store")):
                out.append(ins)
    assert found == 1, found
    return out


def _nt(ins):
    return bool(re.search(r"\bnt\b", ins))


def test_bottom_pass_stream_kernel_tile_accesses_are_non_temporal(code_object):
    mem = _memory_instructions(code_object, BOTTOM_STREAM)
    stores = [i for i in mem if i.startswith("global_store")]
    assert len(stores) == 4 and all(i.startswith("global_store_dwordx4") and _nt(i) for i in stores), stores
    # 16-byte loads: the tile (first column of a run + the prefetch of the next: 4 each) and ONE twiddle vector (layer 1)
    wide = [i for i in mem if i.startswith("global_load_dwordx4")]
    assert sum(_nt(i) for i in wide) == 8 and len(wide) == 9, wide
    assert not [i for i in mem if not i.startswith("global_load_dwordx4") and i.startswith("global_load") and _nt(i)], "twiddle loads keep the default policy"


def test_strided_pass_stream_kernel_tile_accesses_are_non_temporal(code_object):
    mem = _memory_instructions(code_object, STRIDED_STREAM)
    stores = [i for i in mem if i.startswith("global_store")]
    assert stores and all(_nt(i) for i in stores), [i for i in stores if not _nt(i)][:4]
    wide = [i for i in mem if i.startswith("global_load_dwordx4")]
    assert wide and all(_nt(i) for i in wide), [i for i in wide if not _nt(i)][:4]
    assert not [i for i in mem if i.startswith("global_load_dword ") and _nt(i)], "twiddle loads keep the default policy"


@pytest.mark.parametrize("kernel", [BOTTOM, STRIDED, r"k_cfft_bILb1ELi13ELb0E", r"k_cfft_aILb1ELi9ELi0ELi15E"])
def test_default_kernels_keep_the_default_policy(code_object, kernel):
    mem = _memory_instructions(code_object, kernel)
    assert mem and not [i for i in mem if _nt(i)]


@pytest.mark.parametrize("kernel", [BOTTOM, BOTTOM_STREAM])
def test_bottom_pass_resources(code_object, kernel):
    md = _metadata(code_object, kernel)
    assert md["private_segment_fixed_size"] == 0, md
    assert md["max_flat_workgroup_size"] == 1 << (LOGT - 4), md
    assert md["vgpr_count"] <= 80, md                       # 6 waves per SIMD: three 512-lane workgroups per CU
    assert 3 * (md["group_segment_fixed_size"] + DYNAMIC_LDS) <= CU_LDS, md
