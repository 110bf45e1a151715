"""Kernel by kernel: is the code text of two hipcc -S --cuda-device-only listings the same?

    python tools/kernel_text_diff.py before.s after.s [--ops]

A kernel's text = the lines between its label and its .Lfunc_end, comments (';' to the end of the line) and assembler directives
(lines that begin with '.') left out, and the function index of basic-block labels dropped (.LBB12_3 -> .LBB_3: a kernel emitted in
front of the others shifts it). Prints IDENTICAL / DIFFERENT / NEW / GONE per kernel, by demangled name.

--ops: beside every DIFFERENT kernel a verdict and every opcode whose count differs (before->after); an opcode outside the classes that
may change carries its class. The two encodings of one VALU opcode (_e32 / _e64) are counted together; nothing else is merged.
A refactoring that only moves source text may reorder instructions and change the bookkeeping around them, but not the work. These
classes may change count:
    move         v_mov*, v_accvgpr_*, s_mov*
    wait         s_waitcnt, s_nop
    exec/branch  saveexec, 64-bit mask logic, scalar compares and selects, branches
    integer      integer and bit arithmetic (addresses and predicates)
These may not:
    matrix       v_mfma*
    lds          ds_*  (ds_write2_b32 and ds_write_b32 are two opcodes)
    memory       global_*, flat_*, buffer_*, scratch_*, s_load*
    float        any opcode typed f16 / f32 / f64
    select       v_cndmask*
    lane         v_readlane, v_writelane (SGPRs spilled into VGPR lanes)
    other        anything else
Exit status 1 if a kernel is NOT CONFINED to the first four."""
import collections, re, sys, subprocess

MAY_CHANGE = ('move', 'wait', 'exec/branch', 'integer')
CLASSES = (  # first match wins
    ('matrix', r'v_s?mfma'),
    ('lds', r'ds_'),
    ('memory', r'(global|flat|buffer|scratch)_|s_(buffer_)?load'),
    ('float', r'.*_(f16|bf16|f32|f64)(_|$)'),
    ('move', r'v_mov|v_accvgpr_|s_mov'),
    ('select', r'v_cndmask'),
    ('lane', r'v_(read|write)lane'),
    ('wait', r's_waitcnt|s_nop'),
    ('exec/branch', r's_\w+_saveexec_|s_(and|or|xor|andn2|orn2|not|nand|nor|xnor)_b64|s_cmp_|s_cselect_|s_cbranch_|s_branch'),
    ('integer', r'[sv]_(add|addc|sub|subb|subrev|mul|mad|lshl|lshr|ashr|lshlrev|lshrrev|ashrrev|and|or|xor|not|bfe|bfi|min|max|cmp|cmpx)\w*'),
)


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


def opclass(op):
    for name, pat in CLASSES:
        if re.match(pat, op): return name
    return 'other'


def opcounts(lines):
    ops = (ln.split()[0] for ln in lines)
    return collections.Counter(re.sub(r'_e(32|64)$', '', op) for op in ops if not op.endswith(':'))


def compare_ops(before, after):
    """(verdict, confined) for two kernels whose text differs"""
    ca, cb = opcounts(before), opcounts(after)
    changed = sorted(op for op in set(ca) | set(cb) if ca[op] != cb[op])
    if not changed: return 'same opcode counts, another order', True
    classes = {opclass(op) for op in changed}
    outside = sorted(classes - set(MAY_CHANGE))
    listing = ', '.join(f"{op} {ca[op]}->{cb[op]}" + ('' if opclass(op) in MAY_CHANGE else f" [{opclass(op)}]") for op in changed)
    if outside: return f"NOT CONFINED ({', '.join(outside)}): {listing}", False
    return f"confined to {', '.join(sorted(classes))}: {listing}", True


def dem(n):
    return re.sub(r'\(.*', '', subprocess.run(['c++filt', n], capture_output=True, text=True).stdout.strip()).replace('void matinv::', '')


ops = '--ops' in sys.argv[1:]
paths = [p for p in sys.argv[1:] if p != '--ops']
a, b = kernels(paths[0]), kernels(paths[1])
violations = 0
for k in sorted(set(a) | set(b)):
    if k not in a: print(f"NEW        {dem(k)}  ({len(b[k])} lines)")
    elif k not in b: print(f"GONE       {dem(k)}")
    elif a[k] == b[k] or not ops: print(f"{'IDENTICAL' if a[k] == b[k] else 'DIFFERENT'}  {dem(k)}  ({len(a[k])} / {len(b[k])} lines)")
    else:
        verdict, confined = compare_ops(a[k], b[k])
        violations += not confined
        print(f"DIFFERENT  {dem(k)}  ({len(a[k])} / {len(b[k])} lines)  {verdict}")
if ops:
    print(f"{violations} kernel(s) with a change outside {', '.join(MAY_CHANGE)}")
    sys.exit(1 if violations else 0)
