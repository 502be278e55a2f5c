"""Compares the gfx950 machine code of two builds kernel by kernel (CPU only; nothing is executed):

    python tools/isa_compare.py PARENT_OBJ_DIR BRANCH_OBJ_DIR [translation unit ...]

The code objects are taken out of the object files and disassembled the way tests/test_cpu_isa.py does (its _disasm is reused).  A
kernel is looked up by its mangled name in ANY of the named translation units of a side (default: every *.o of the directory), so a
kernel that moved to another source file is still compared with itself.  One line per kernel: `same` when the instruction lists
(addresses and branch-target annotations stripped, everything behind the last s_endpgm ignored: the fill between kernels depends on
what follows in the object) and the vgpr / sgpr / LDS / scratch notes are equal, `DIFF` with both figures otherwise, `only-parent` /
`only-branch` for a kernel one side lacks.  Exit status 1 unless every line says `same`."""
import os
import pathlib
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import test_cpu_isa as isa  # noqa: E402

NOTES = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def _notes(code_object):
    """{kernel symbol: (vgpr, sgpr, LDS bytes, scratch bytes)} from the amdhsa.kernels list of the code object's metadata note."""
    text = subprocess.check_output([os.path.join(isa.LLVM, "llvm-readelf"), "--notes", code_object], text=True)
    lines = text.splitlines()
    out, cur, dash = {}, None, None            # dash: column of the "- " that opens an entry of the list

    def close():
        if cur is not None:
            out[cur["symbol"][:-len(".kd")]] = tuple(int(cur[k]) for k in NOTES)      # KeyError: a note this script relies on is missing

    for i, line in enumerate(lines):
        if line.strip() == "amdhsa.kernels:":
            dash = lines[i + 1].index("-")
            continue
        if dash is None:
            continue
        indent = len(line) - len(line.lstrip())
        if line.strip() and indent < dash:        # the list is over
            break
        if indent == dash and line[dash] == "-":  # the next kernel
            close()
            cur = {}
        m = re.match(r"^[ -]{%d}\.(\w+):\s+(\S+)$" % (dash + 2), line)      # kernel-level keys only (argument keys sit deeper)
        if m:
            cur[m.group(1)] = m.group(2)
    close()
    return out


def _kernel_symbols(code_object):
    """The kernels of the code object by its symbol table (every kernel has a descriptor NAME.kd), independent of the notes."""
    text = subprocess.check_output([os.path.join(isa.LLVM, "llvm-readelf"), "--symbols", "--wide", code_object], text=True)
    return {m.group(1) for m in re.finditer(r"(\S+)\.kd$", text, re.M)}


def kernels_of(obj_dir, tus):
    """{mangled name: (translation unit, [instructions], notes)} over the translation units `tus` of obj_dir."""
    isa.OBJ = obj_dir            # _disasm reads the test module's object directory: point it at the side being read
    out = {}
    for tu in tus:
        sections = subprocess.check_output([os.path.join(isa.LLVM, "llvm-readelf"), "-S", os.path.join(obj_dir, tu + ".o")], text=True)
        if ".hip_fatbin" not in sections:         # host code only (gkr_prove): no code object, no kernels
            continue
        with tempfile.TemporaryDirectory() as tmp:
            code = isa._disasm(tu, pathlib.Path(tmp))
            notes = _notes(os.path.join(tmp, "dev.co"))
            names = _kernel_symbols(os.path.join(tmp, "dev.co"))
        lost = sorted(n for n in names if n not in notes or n not in code)
        if lost:
            sys.exit(f"{obj_dir}/{tu}.o: kernels without notes or code in the dump: {lost}")
        for name in names:
            ins = code[name]
            last = max(i for i, x in enumerate(ins) if x.split()[0] == "s_endpgm")
            out[name] = (tu, ins[:last + 1], notes[name])
    return out


_short_names = {}


def _short(name):
    """k_merkle_upq<256> for _ZN12_GLOBAL__N_112k_merkle_upqILi256EEEv...; the mangled name where binutils' c++filt is missing."""
    if name not in _short_names:
        filt = shutil.which("c++filt")
        full = subprocess.check_output([filt, name], text=True).strip() if filt else name
        _short_names[name] = re.sub(r"^void ", "", full.replace("(anonymous namespace)::", "")).split("(")[0]
    return _short_names[name]


def main(argv):
    parent_dir, branch_dir, tus = argv[0], argv[1], argv[2:]
    sides = []
    for d in (parent_dir, branch_dir):
        have = sorted(f[:-2] for f in os.listdir(d) if f.endswith(".o"))
        sides.append(kernels_of(d, [t for t in have if not tus or t in tus]))
    parent, branch = sides
    bad = 0
    for name in sorted(set(parent) | set(branch), key=_short):
        p, b = parent.get(name), branch.get(name)
        if p is None or b is None:
            status, detail = ("only-parent" if b is None else "only-branch"), (p or b)[0] + ".o"
        else:
            same = p[1] == b[1] and p[2] == b[2]
            status = "same" if same else "DIFF"
            detail = f"{p[0]}.o -> {b[0]}.o  instructions {len(p[1])} -> {len(b[1])}  vgpr/sgpr/lds/scratch {p[2]} -> {b[2]}"
        bad += status != "same"
        print(f"{status:11s} {_short(name):45s} {detail}")
    print(f"{len(set(parent) | set(branch))} kernels, {bad} not the same")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
