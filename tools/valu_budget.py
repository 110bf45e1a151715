"""Static instruction budget of one kernel in a hipcc -S --cuda-device-only listing.

    python tools/valu_budget.py file.s [kernel-substring ...]

The default kernel is the headline matinv_gj_tile_f64<4, true, true, false>. Its block steps are fully unrolled, so the
static counts are per-matrix counts (the grid-stride loop runs the body once per matrix). VALU = every v_* instruction,
the MFMAs included (that is what SQ_INSTS_VALU counts); "non-MFMA VALU" leaves them out. Registers and scratch are read
from the listing's .set lines, as tools/kernel_regs.py does.
"""
import re, sys
from collections import Counter

HEADLINE = "_ZN6matinv18matinv_gj_tile_f64ILi4ELb1ELb1ELb0EE"

ROWS = [
    ("v_mfma_*", lambda op, src: op.startswith("v_mfma")),
    ("v_fma/fmac/mul/rcp/add_f64", lambda op, src: re.match(r"v_(fma|fmac|mul|rcp|add)_f64", op) is not None),
    ("v_fma/fmac/mul/rcp/add_f32", lambda op, src: re.match(r"v_(fma|fmac|mul|rcp|add)_f32", op) is not None),
    ("v_mov_*_dpp (lane broadcast)", lambda op, src: op.startswith("v_mov") and op.endswith("_dpp")),
    ("v_mov_b64 ..., 0", lambda op, src: op.startswith("v_mov_b64") and src == "0"),
    ("v_mov_b64 vX, vY (copy)", lambda op, src: op.startswith("v_mov_b64") and src.startswith("v[")),
    ("v_mov_b32 ..., 0 / const", lambda op, src: op.startswith("v_mov_b32") and not src.startswith(("v", "s"))),
    ("v_mov_b32 vX, vY (copy)", lambda op, src: op.startswith("v_mov_b32") and re.match(r"v\d", src) is not None),
    ("v_mov_b32 vX, sY", lambda op, src: op.startswith("v_mov_b32") and src.startswith("s")),
    ("v_cndmask_b32", lambda op, src: op.startswith("v_cndmask")),
    ("v_cmp*", lambda op, src: op.startswith("v_cmp")),
    ("v_xor_b32", lambda op, src: op.startswith("v_xor")),
]


def kernel_body(text, key):
    m = re.search(r"^(" + re.escape(key) + r"\S*):", text, re.M) if key.startswith("_Z") else None
    if m is None:
        m = re.search(r"^(_Z\S*" + re.escape(key) + r"\S*):", text, re.M)
    if m is None:
        sys.exit(f"kernel {key!r} not found")
    name = m.group(1)
    end = text.index(".Lfunc_end", m.end())
    return name, text[m.end():end]


def budget(text, key):
    name, body = kernel_body(text, key)
    rows, other = Counter(), Counter()
    valu = snop = snop_cycles = 0
    for line in body.splitlines():
        line = line.split(";")[0].strip()
        if not line or line.endswith(":") or line.startswith("."):
            continue
        parts = line.split(None, 1)
        op = parts[0]
        args = [x.strip() for x in parts[1].split(",")] if len(parts) > 1 else []
        if op == "s_nop":
            snop += 1
            snop_cycles += int(args[0], 0) + 1
            continue
        if not op.startswith("v_"):
            continue
        valu += 1
        src = args[1] if len(args) > 1 else ""
        for label, pred in ROWS:
            if pred(op, src):
                rows[label] += 1
                break
        else:
            other[op] += 1
    sets = dict(re.findall(re.escape(name) + r"\.(\w+), (\d+)", text))
    return name, rows, other, valu, snop, snop_cycles, sets


def main():
    path = sys.argv[1]
    keys = sys.argv[2:] or [HEADLINE]
    text = open(path).read()
    for key in keys:
        name, rows, other, valu, snop, snop_cycles, sets = budget(text, key)
        print(name)
        print(f"  vgpr {sets.get('num_vgpr')}  agpr {sets.get('num_agpr')}  scratch {sets.get('private_seg_size')}")
        for label, _ in ROWS:
            print(f"  {label:30s} {rows[label]:6d}")
        print(f"  {'other VALU':30s} {sum(other.values()):6d}   " + " ".join(f"{k}:{v}" for k, v in other.most_common(8)))
        print(f"  {'VALU total':30s} {valu:6d}")
        print(f"  {'non-MFMA VALU':30s} {valu - rows['v_mfma_*']:6d}")
        print(f"  {'s_nop (wait states)':30s} {snop:6d}   ({snop_cycles} cycles)")


if __name__ == "__main__":
    main()
