#!/usr/bin/env python3
"""Every kernel that libmatinv_hip.so ships, with its register budget: python tools/library_kernels.py [--digest] [path/to/libmatinv_hip.so]
(llvm-objdump --offloading on a copy of the library in a temporary directory, llvm-readelf --notes on the gfx950 code objects.)
regs = VGPRs + AGPRs of one lane (unified file: 512 / waves per SIMD), agpr = the AGPR part, scratch in bytes per lane.
--digest: also the number of code objects that hold each kernel and a hash of its disassembly (llvm-objdump -d without raw bytes or
addresses, encodings, padding and symbolised <...> branch annotations). Two builds with equal digests ship the same device code: diff the outputs
to check that a host-side change left every kernel as it was."""
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
args = [a for a in sys.argv[1:] if a != "--digest"]
digest = len(args) < len(sys.argv) - 1
so = args[0] if args else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda-matrix-inversion_amd", "libmatinv_hip.so")


def bodies(code_object):
    """mangled kernel name -> hash of its disassembly"""
    t = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", code_object],
                       capture_output=True, text=True, check=True).stdout
    out = {}
    for m in re.finditer(r"^<(\S+)>:\n(.*?)(?=^<\S+>:\n|\Z)", t, re.S | re.M):
        # the AMDGPU disassembler still prints "// address: encoding" after each instruction: drop it with the <...> annotations, and
        # the "..." of the zero padding behind a kernel (it depends on where the kernel sits in its code object)
        body = re.sub(r"[ \t]*(//[^\n]*|<[^>\n]*>)|^\s*\.\.\.\s*$", "", m.group(2), flags=re.M).strip()
        out[m.group(1)] = hashlib.sha256(body.encode()).hexdigest()[:16]
    return out


with tempfile.TemporaryDirectory() as tmp:
    lib = shutil.copy(so, os.path.join(tmp, "lib.so"))
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", lib], capture_output=True, text=True, cwd=tmp)
    rows, objects, hashes = [], {}, {}
    for f in sorted(glob.glob(os.path.join(tmp, "*gfx950"))):
        t = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", f], capture_output=True, text=True).stdout
        h = bodies(f) if digest else {}
        for m in re.finditer(r"\.agpr_count:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?"
                             r"\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", t, re.S):
            name = m.group(2)
            objects[name] = objects.get(name, 0) + 1
            if digest and objects[name] > 1:
                hashes[name] += "," + h.get(name, "-")
                continue
            hashes[name] = h.get(name, "-")
            rows.append((name, int(m.group(5)), int(m.group(1)), int(m.group(3)), int(m.group(6)), int(m.group(4))))
names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.splitlines()
out = []
for r, nm in zip(rows, names):
    nm = re.sub(r"\((?!anonymous namespace\)).*", "", nm).replace("void matinv::", "")
    line = f"{nm:66s} regs {r[1]:4d}  agpr {r[2]:3d}  scratch {r[3]:5d}  spilled {r[4]:4d}"
    if digest:
        line += f"  sgpr {r[5]:3d}  objects {objects[r[0]]}  body {hashes[r[0]]}"
    out.append(line)
print(f"# {len(out)} kernels in {os.path.basename(so)}" + ("" if digest else f" ({os.path.getsize(so)} bytes)"))
print("\n".join(sorted(out)))
