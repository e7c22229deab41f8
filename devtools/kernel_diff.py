#!/usr/bin/env python3
"""Dev tool: are the kernels of two builds the same code?

    python devtools/kernel_diff.py BEFORE_DIR AFTER_DIR [object.o ...]

BEFORE_DIR and AFTER_DIR hold object files of the same names built from two trees with build.py's flags (by default kernels_pyramid.o
and kernels_expand_sd.o: copy <package>/build/ of the parent commit aside, rebuild, compare). For every kernel of an object's gfx950
code object — the kernels are the entries of its metadata note — the tool compares

  * the disassembled body (build._kernel_bodies: llvm-objdump -d of the code object) without the address and encoding column: branches
    are relative, so where a kernel sits in the file does not show;
  * .vgpr_count, .sgpr_count, .private_segment_fixed_size (scratch) and .group_segment_fixed_size (LDS) of the metadata

and prints one line per kernel: object, name, the four numbers (before -> after where they differ), the instruction count, `same` or
`DIFFERENT`. A kernel found on one side only, or in another object file than before, is `MISSING` / `NEW`. Exit status 1 unless
everything is `same`. It compares only: it looks for no particular instruction."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import build  # noqa: E402

FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(obj):
    """{mangled name: (the four metadata numbers, body lines without the address / encoding comment)} of one object file"""
    listing, notes = build._code_object_text(obj, ("llvm-objdump", "-d"), ("llvm-readobj", "--notes"))
    meta, cur, indent = {}, None, None
    for line in notes.splitlines():
        m = re.match(r"^(\s*)(- )?(\.\w+):\s*(.*)$", line)
        if not m:
            if line.startswith("amdhsa.kernels:"):
                indent = -1
            elif indent is not None and re.match(r"^\S", line):
                indent = None   # the next top-level key: the list of kernels is over
            continue
        if indent is None:
            continue
        if m.group(2) and (indent == -1 or len(m.group(1)) == indent):   # a new entry of the list of kernels (its arguments' entries sit deeper)
            indent = len(m.group(1))
            cur = {}
        if len(m.group(1)) + (2 if m.group(2) else 0) == indent + 2:
            cur[m.group(3)] = m.group(4).strip().strip("'\"")
            if m.group(3) == ".name":
                meta[cur[".name"]] = cur
    bodies = {}
    for label, body in build._kernel_bodies(listing).items():
        name = label[label.index("<") + 1:-2]
        bodies[name] = [re.sub(r"\s*//.*$", "", l).strip() for l in body if l.strip()]
    return {name: (tuple(int(d.get(f, -1)) for f in FIELDS), bodies.get(name, [])) for name, d in meta.items()}


def main(argv):
    if len(argv) < 3:
        raise SystemExit(__doc__)
    before_dir, after_dir = argv[1], argv[2]
    objs = argv[3:] or ["kernels_pyramid.o", "kernels_expand_sd.o"]
    different = 0
    print("%-22s %-72s %5s %5s %7s %6s %6s  %s" % ("object", "kernel", "vgpr", "sgpr", "scratch", "lds", "instr", ""))
    for o in objs:
        a, b = kernels(os.path.join(before_dir, o)), kernels(os.path.join(after_dir, o))
        for name in list(a) + [n for n in b if n not in a]:
            if name not in a or name not in b:
                (ma, body), verdict = (a[name], "MISSING") if name in a else (b[name], "NEW")
                mb = ma
            else:
                (ma, body), (mb, body_b) = a[name], b[name]
                verdict = "same" if ma == mb and body == body_b and body else "DIFFERENT"
            different += verdict != "same"
            cols = ["%d" % x if x == y else "%d->%d" % (x, y) for x, y in zip(ma, mb)]
            print("%-22s %-72s %5s %5s %7s %6s %6d  %s" % (o, name, cols[0], cols[1], cols[2], cols[3], len(body), verdict))
    print("%d kernel(s) not the same" % different if different else "every kernel the same")
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
