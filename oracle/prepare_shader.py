#!/usr/bin/env python3
"""Prepare one of the reference's compute shaders for a C++ front end.

    prepare_shader.py IN.comp OUT.inc

The output lands in oracle/_ref/gen/ (git-ignored) and is included by
ref_shaders.cpp behind glsl_host.h. The step changes only what a C++ compiler
cannot parse; every expression, loop and branch of the shader stays as written:

  1. `#version ...` is dropped.
  2. An interface block `layout(...) [readonly] buffer|uniform Name { members };`
     becomes its member declarations at the shader's scope, so the members are
     visible unqualified, as GLSL makes them. The entry point in ref_shaders.cpp
     copies the caller's block in before the dispatch and out after it.
  3. `layout(local_size_x = A, local_size_y = B) in;` becomes
     `enum { local_size_x = A, local_size_y = B };` (a missing axis is 1), which
     the dispatcher reads. Every other `layout(...)` qualifier becomes nothing:
     bindings and image formats are the host's business, so a wrong format
     qualifier as in clahe_histogram.comp:10 cannot matter.
  4. The storage qualifiers `uniform`, `readonly`, `writeonly` become nothing.
  5. The constant rule (glsl_host.h, "number model"): a scalar
     `const float NAME = E;` becomes `const auto NAME = glsl_const(E);`, so a
     constant initialiser keeps glslang's double and a run-time one stays a float.
  6. Every macro the shader defines is undefined again at the end, so the next
     shader in the same translation unit starts clean.
"""
import re
import sys

BLOCK = re.compile(
    r"layout\s*\([^)]*\)\s*(?:readonly\s+|writeonly\s+)?(?:buffer|uniform)\s+(?:readonly\s+|writeonly\s+)?\w+\s*\{([^}]*)\}\s*;")
LAYOUT_IN = re.compile(r"layout\s*\(([^)]*)\)\s*in\s*;")
LAYOUT = re.compile(r"layout\s*\([^)]*\)")
QUALIFIER = re.compile(r"\b(?:uniform|readonly|writeonly)\b")
CONST_FLOAT = re.compile(r"\bconst\s+float\s+(\w+)\s*=\s*([^;\[\]{}]+);")
VERSION = re.compile(r"^\s*#\s*version\b.*$", re.M)
DEFINE = re.compile(r"^\s*#\s*define\s+(\w+)", re.M)


def local_size(m):
    sizes = {"local_size_x": "1", "local_size_y": "1"}
    for part in m.group(1).split(","):
        key, value = part.split("=")
        sizes[key.strip()] = value.strip()
    return "enum { local_size_x = %s, local_size_y = %s };" % (sizes["local_size_x"], sizes["local_size_y"])


def prepare(text):
    text = VERSION.sub("", text)
    text = BLOCK.sub(lambda m: m.group(1), text)
    text = LAYOUT_IN.sub(local_size, text)
    text = LAYOUT.sub("", text)
    text = QUALIFIER.sub("", text)
    text = CONST_FLOAT.sub(lambda m: "const auto %s = glsl_const(%s);" % (m.group(1), m.group(2).strip()), text)
    names = []
    for n in DEFINE.findall(text):
        if n not in names:
            names.append(n)
    return text + "\n" + "".join("#undef %s\n" % n for n in names)


if __name__ == "__main__":
    with open(sys.argv[1], "r", encoding="utf-8", errors="replace") as f:
        src = f.read()
    with open(sys.argv[2], "w", encoding="utf-8") as f:
        f.write(prepare(src))
