"""Kernel-by-kernel comparison of the gfx950 instructions of two builds of libbsched.so: every code object of each library (one offload
bundle per translation unit) is disassembled (llvm-objdump -d, addresses, raw bytes, comments and branch-target offsets stripped) and
the kernels are compared by name.  Usage: python tools/isa_diff.py OLD.so NEW.so — prints one summary line, then one line per kernel
that differs; exit status 1 when a kernel differs or is in one library only.

objdump prints the zero fill behind the last s_endpgm of a section as a line `...`: it belongs to whichever kernel the compiler emitted
last, which changes with the order of instantiation and says nothing about the kernel, so the line is dropped.  The same holds for the
run of `s_nop 0` that pads the end of a code object's .text section (where the non-template kernels sit): it lands on whichever of them is
last in its unit, so moving a kernel family to another unit moves the padding; no kernel's own code ends in `s_nop 0`, and a trailing run
of them is dropped from every kernel."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernels(lib):
    """{symbol: "hash of the instruction text:instruction count"} over every code object of the library"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat")
        # (an output file of its own: with the input alone, objcopy writes its copy back over the library)
        subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(d, "copy")], check=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for n, a in enumerate(starts):
            part, co = os.path.join(d, f"fat{n}"), os.path.join(d, f"co{n}")
            open(part, "wb").write(blob[a:(starts[n + 1] if n + 1 < len(starts) else len(blob))])
            subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={part}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            f"--output={co}"], check=True)
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], capture_output=True, text=True, check=True).stdout
            text, cur = {}, None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line)
                if m:
                    cur = m.group(1)
                    assert cur not in text and cur not in out, f"{cur} is emitted twice"
                    text[cur] = []
                    continue
                ins = re.sub(r"<\S+\+0x[0-9a-f]+>", "", re.sub(r"//.*$", "", line)).strip()
                if cur and ins and ins != "...":
                    text[cur].append(ins)
            for k, v in text.items():
                while v and v[-1] == "s_nop 0":
                    v.pop()
                out[k] = hashlib.md5("\n".join(v).encode()).hexdigest()[:12] + ":" + str(len(v))
    return out


if __name__ == "__main__":
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    diff = sorted(k for k in a if k in b and a[k] != b[k])
    only_old, only_new = sorted(k for k in a if k not in b), sorted(k for k in b if k not in a)
    print("kernels old", len(a), "new", len(b), "same", sum(1 for k in a if k in b and a[k] == b[k]), "diff", len(diff), "only old", only_old, "only new", only_new)
    for k in diff:
        print("DIFF", k, a[k], b[k])
    sys.exit(1 if diff or only_old or only_new else 0)
