#!/usr/bin/env python3
"""Dev tool (round 9): the instruction-class table of a kernel's hot loop, from a device listing.

    hipcc --offload-arch=gfx950 <build.py's flags for the file> -x hip -S --cuda-device-only csrc/kernels_expand_sd.hip -o /tmp/x/expand_sd.s
    python devtools/isa_classes.py /tmp/x/expand_sd.s k_expand_fastILi2ELb1ELb1ELi3ELb0ELb1E --texels 48 --loop 8
    (k_expand_fast holds one march per LUTOK / CNR48 case: loop 8 is the LUTOK && CNR48 march real images run, the largest loop — what
    the tool picks without --loop — is the literal curve scan of degenerate curves. The loops are listed first; name the one meant.)

The kernel is the first one whose (mangled) label contains the given string. A loop is a backward branch: the lines from its target
label to the branch. Loops that lie inside another are folded into the outermost one; the table is that of the loop with the most
vector instructions unless --loop picks another (they are listed first, in source order). Only ordinary vector (v_*), LDS (ds_*) and
memory (buffer_ / global_ / flat_ / scratch_) opcodes are counted: scalar instructions, waits and labels are not. Basic blocks that
hold one of --cold's opcodes (the literal sqrtf(x / 25) fall-back of exact_math.h, laid out behind the loop's back edge) are left out.
--texels N adds the per-texel column (the SD march's loop holds three trips of 16 texels per lane: 48)."""
import argparse
import re
import sys

CLASSES = (
    ("float arithmetic", re.compile(r"^v_(mul|add|sub|subrev|fma|fmac|mac|mad)_(f32|legacy_f32)|^v_pk_(mul|add|fma)_f32")),
    ("float min / max / med3", re.compile(r"^v_(min|max|med3|min3|max3)_f32")),
    ("v_rsq + conversions", re.compile(r"^v_(rsq|rcp|sqrt|cvt|floor|trunc|rndne|fract)_")),
    ("compares", re.compile(r"^v_cmpx?_")),
    ("v_cndmask", re.compile(r"^v_cndmask_")),
    ("v_mov", re.compile(r"^v_mov_|^v_accvgpr_")),
    ("integer ALU", re.compile(r"^v_(and|or|xor|not|lshl|lshr|ashr|add|sub|subrev|addc|subb|subbrev|bfe|bfi|bfm|perm|alignbit|alignbyte|mul|mad|min|max|med3|min3|max3|or3|and_or|lshl_or|lshl_add|add_lshl|add3|xad|sad|dot\d)_?")),
    ("LDS", re.compile(r"^ds_")),
    ("memory", re.compile(r"^(buffer|global|flat|scratch)_")),
)
FLOAT_DETAIL = ("v_mul", "v_add", "v_sub", "v_fma", "v_fmac")


def kernel_lines(path, name):
    body, state, label = [], "before", None
    with open(path) as f:
        for line in f:
            s = line.strip()
            if state == "before":
                if re.match(r"^[A-Za-z_][\w$.]*:", s) and name in s.split(":")[0]:
                    state, label = "code", s.split(":")[0]
                continue
            if s.startswith(".Lfunc_end"):
                state = "tail"   # the resource comments (; NumVgprs ...) follow the function's end; the next kernel's label ends them
            elif state == "tail" and re.match(r"^[A-Za-z_][\w$.]*:", s):
                break
            body.append(s)
    if label is None:
        raise SystemExit("no kernel whose label contains %r in %s" % (name, path))
    return label, body


def opcode(s):
    if not s or s[0] in ".;" or s.endswith(":"):
        return None
    return s.split()[0]


def classify(op):
    for cname, rx in CLASSES:
        if rx.match(op):
            return cname
    return "other vector" if op.startswith("v_") else None


def loops(body):
    at = {}
    for i, s in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            at[m.group(1)] = i
    spans = []
    for i, s in enumerate(body):
        m = re.match(r"^s_c?branch\S*\s+(\.LBB\d+_\d+)", s)
        if m and m.group(1) in at and at[m.group(1)] < i:
            spans.append((at[m.group(1)], i))
    spans.sort(key=lambda t: (t[0], -t[1]))
    outer = []
    for lo, hi in spans:
        if outer and lo <= outer[-1][1]:
            outer[-1] = (outer[-1][0], max(outer[-1][1], hi))
        else:
            outer.append((lo, hi))
    return outer


def drop_blocks(lines, cold):
    """The lines without the basic blocks (label to label) that hold one of the `cold` opcodes: the literal sqrtf / division fall-backs
    of the exact-math helpers are laid out inside the loop and never run on ordinary images."""
    out, block = [], []
    def flush():
        if not any(opcode(s) in cold for s in block):
            out.extend(block)
    for s in lines:
        if re.match(r"^\.LBB\d+_\d+:", s):
            flush()
            block = []
        block.append(s)
    flush()
    return out


def count(lines):
    c, detail = {}, {}
    for s in lines:
        op = opcode(s)
        if not op:
            continue
        k = classify(op)
        if k is None:
            continue
        c[k] = c.get(k, 0) + 1
        detail.setdefault(k, {})
        detail[k][op] = detail[k].get(op, 0) + 1
    return c, detail


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("kernel")
    ap.add_argument("--texels", type=int, default=0, help="texels per lane and loop iteration, for the per-texel column")
    ap.add_argument("--loop", type=int, default=-1, help="index of the loop to tabulate (default: the one with the most vector instructions)")
    ap.add_argument("--ops", action="store_true", help="list the opcodes of every class")
    ap.add_argument("--cold", default="v_sqrt_f32_e32", help="opcodes that mark a basic block as a cold fall-back, left out of the counts ('' keeps all)")
    a = ap.parse_args()
    label, body = kernel_lines(a.listing, a.kernel)
    meta = {}
    for s in body:
        m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize|NumSgprs)\S*:?\s*(\d+)", s) or re.match(r"^; (codeLenInByte) = (\d+)", s)
        if m and m.group(1) not in meta:
            meta[m.group(1)] = int(m.group(2))
    print("kernel %s" % label)
    print("  " + "  ".join("%s %d" % kv for kv in meta.items()))
    ls = loops(body)
    if not ls:
        raise SystemExit("no loop found")
    cold = set(x for x in a.cold.split(",") if x)
    sizes = []
    for n, (lo, hi) in enumerate(ls):
        c, _ = count(drop_blocks(body[lo:hi + 1], cold))
        sizes.append(sum(c.values()))
        print("  loop %d: listing lines %d..%d of the kernel, %d vector / LDS / memory instructions" % (n, lo, hi, sizes[-1]))
    pick = a.loop if a.loop >= 0 else max(range(len(ls)), key=lambda n: sizes[n])
    lo, hi = ls[pick]
    c, detail = count(drop_blocks(body[lo:hi + 1], cold))
    total = sum(c.values())
    per = (lambda v: "%6.1f" % (v / a.texels)) if a.texels else (lambda v: "")
    print("loop %d: %d vector, LDS and memory instructions%s" % (pick, total, (", %.1f per texel" % (total / a.texels)) if a.texels else ""))
    print("  %-26s %8s %s" % ("class", "per loop", "per texel" if a.texels else ""))
    for cname in [n for n, _ in CLASSES] + ["other vector"]:
        v = c.get(cname, 0)
        extra = ""
        if cname == "float arithmetic":
            d = detail.get(cname, {})
            extra = "   (" + ", ".join("%s %d" % (p, sum(v2 for o, v2 in d.items() if re.match(p + r"(rev)?_", o))) for p in FLOAT_DETAIL) + ")"
        print("  %-26s %8d %s%s" % (cname, v, per(v), extra))
        if a.ops:
            for o, v2 in sorted(detail.get(cname, {}).items(), key=lambda t: -t[1]):
                print("      %-28s %6d" % (o, v2))
    book = sum(c.get(k, 0) for k in ("compares", "v_cndmask", "integer ALU", "v_mov"))
    print("  %-26s %8d %s" % ("bookkeeping (cmp+cnd+int+mov)", book, per(book)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
