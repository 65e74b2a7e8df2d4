"""The kernel-argument layout of built device code, read from the code objects themselves: for every kernel the offsets, sizes and
kinds of its arguments (the AMDGPU metadata note) and the preload length of its kernel descriptor.

    python tools/kernarg_layout.py [files ...]        default: asset_asrl_amd/csrc/obj/tu_reentry_lgl4_0.o

Files: whatever tools/isa_dpp_hazard.py reads -- host objects / shared objects with a .hip_fatbin section, raw code objects, the cache
files of the in-process compiler.  Prints one line per kernel that takes the parameter list of csrc/eval_args.h (its name contains the
EvalCold struct): preload length, explicit arguments as offset:size.  tests/test_kernarg_layout_cpu.py holds these against what
eval_args_pack writes.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_dpp_hazard import LLVM, ROOT, RTC_MAGIC, TARGET  # noqa: E402

EVAL_MARK = "NS_8EvalColdE"          # the by-value struct of ASSET_EVAL_PARAMS in a mangled kernel name


def code_objects(path, td):
    """The gfx950 code objects `path` holds, as files under `td`."""
    data = open(path, "rb").read()
    if data.startswith(RTC_MAGIC):                  # header lines, then the code object (capi.hip: rtc_write)
        pos = len(RTC_MAGIC)
        nl = data.index(b"\n", pos)
        for _ in range(int(data[pos:nl]) + 1):
            pos = nl + 1
            nl = data.index(b"\n", pos)
        size = int(data[pos:nl])
        co = os.path.join(td, "rtc.co")
        open(co, "wb").write(data[nl + 1:nl + 1 + size])
        return [co]
    sections = subprocess.run([f"{LLVM}/llvm-objdump", "-h", path], capture_output=True, text=True).stdout
    if ".hip_fatbin" not in sections:
        return [path]
    fat = os.path.join(td, "fat")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", path], stderr=subprocess.DEVNULL)
    blob, out, pos, k = open(fat, "rb").read(), [], 0, 0
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    while True:                                     # a shared object holds one bundle per translation unit, 4 KiB aligned
        pos = blob.find(magic, pos)
        if pos < 0:
            break
        nxt = blob.find(magic, pos + 1)
        one, co = os.path.join(td, f"bundle{k}"), os.path.join(td, f"co{k}")
        open(one, "wb").write(blob[pos:nxt if nxt > 0 else len(blob)])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={one}", f"--targets={TARGET}",
                               f"--output={co}"], stderr=subprocess.DEVNULL)
        if os.path.getsize(co) > 0:
            out.append(co)
        pos, k = pos + 1, k + 1
    return out


def kernels_of(co):
    """{kernel name: {"args": [(offset, size, value_kind)], "preload": dwords}} of one code object."""
    notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True)
    out, args, cur = {}, None, None
    for line in notes.splitlines():
        s = line.strip()
        if s.startswith("- .agpr_count") or s.startswith("- .args") or re.match(r"^  - \.", line):
            args, cur = [], None                    # a new entry of amdhsa.kernels
        if args is None:
            continue
        m = re.match(r"-? *\.offset: +(\d+)", s)
        if m:
            cur = [int(m.group(1)), None, None]
            args.append(cur)
        m = re.match(r"\.size: +(\d+)", s)
        if m and cur is not None and cur[1] is None:
            cur[1] = int(m.group(1))
        m = re.match(r"\.value_kind: +(\S+)", s)
        if m and cur is not None and cur[2] is None:
            cur[2] = m.group(1)
        m = re.match(r"^    \.name: +(\S+)", line)
        if m:
            out[m.group(1)] = {"args": [tuple(a) for a in args], "preload": None}
            args = None
    kd = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "-j", ".rodata", co], text=True)
    name = None
    for line in kd.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)\.kd>:", line)
        if m:
            name = m.group(1)
            if name in out:
                out[name]["preload"] = 0           # (the disassembler prints the directive only for a length that is not zero)
        m = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", line)
        if m and name in out:
            out[name]["preload"] = int(m.group(1))
    return out


def kernels(path):
    res = {}
    with tempfile.TemporaryDirectory() as td:
        for co in code_objects(path, td):
            res.update(kernels_of(co))
    return res


def explicit(args):
    return [(o, s) for o, s, k in args if not k.startswith("hidden_")]


def main(argv):
    files = argv or [os.path.join(ROOT, "asset_asrl_amd", "csrc", "obj", "tu_reentry_lgl4_0.o")]
    for f in files:
        ks = kernels(f)
        n = 0
        for name, k in sorted(ks.items()):
            if EVAL_MARK in name:
                n += 1
                print(f"{os.path.basename(f)}: preload {k['preload']:2d}  " + " ".join(f"{o}:{s}" for o, s in explicit(k["args"])) + f"  {name[:90]}")
        print(f"{os.path.basename(f)}: {len(ks)} kernels, {n} with the evaluation parameter list")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
