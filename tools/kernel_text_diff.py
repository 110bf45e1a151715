"""Kernel by kernel: is the code text of two hipcc -S --cuda-device-only listings the same?

    python tools/kernel_text_diff.py before.s after.s

A kernel's text = the lines between its label and its .Lfunc_end, comments (';' to the end of the line) and assembler directives
(lines that begin with '.') left out, and the function index of basic-block labels dropped (.LBB12_3 -> .LBB_3: a kernel emitted in
front of the others shifts it). Prints IDENTICAL / DIFFERENT / NEW / GONE per kernel, by demangled name."""
import re, sys, subprocess
def kernels(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r'^(_Z\w+):', ln)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if ln.startswith('.Lfunc_end'):
            cur = None
            continue
        if cur is None: continue
        ln = re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r';.*', '', ln)).strip()
        if ln and not ln.startswith('.'): cur.append(ln)
    return {k: v for k, v in out.items() if v}
a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
def dem(n): return re.sub(r'\(.*', '', subprocess.run(['c++filt', n], capture_output=True, text=True).stdout.strip()).replace('void matinv::','')
for k in sorted(set(a) | set(b)):
    if k not in a: print(f"NEW        {dem(k)}  ({len(b[k])} lines)")
    elif k not in b: print(f"GONE       {dem(k)}")
    else: print(f"{'IDENTICAL' if a[k]==b[k] else 'DIFFERENT'}  {dem(k)}  ({len(a[k])} / {len(b[k])} lines)")
