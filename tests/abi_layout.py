"""The layout check of the ctypes mirrors of include/mcgpu_amd.h, shared by the tests of the entry points that take them: for a
list of (struct name in the header, ctypes.Structure mirror) pairs, the header's field names in order, and sizeof plus every field's
offsetof and size as the C compiler lays the header out, against the mirror.  A swap of two fields of one type keeps every size and
offset and is caught only by the names."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

HEADER = Path(__file__).resolve().parents[1] / "include" / "mcgpu_amd.h"


def c_compiler():
    for cc in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang"):
        if shutil.which(cc):
            return shutil.which(cc)
    return None


def header_fields(struct):
    """Field names of `typedef struct <struct> { ... } <struct>;` in the header, in order."""
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S)
    assert body, struct
    names = []
    for decl in body.group(1).split(";"):
        parts = [re.sub(r"\[.*?\]", "", p).replace("*", " ").split() for p in decl.split(",")]
        if parts[0]:
            names += [parts[0][-1]] + [p[0] for p in parts[1:]]
    return names


def assert_field_names(mirrors):
    for struct, cls in mirrors:
        assert header_fields(struct) == [f[0] for f in cls._fields_], struct


def assert_sizes_and_offsets(mirrors, cc, tmp_path):
    """Compiles a program that prints sizeof and every offsetof / field size, asserts them equal to the mirrors' and returns them:
    {"<struct>": "<sizeof>", "<struct>.<field>": "<offset> <size>"}."""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "mcgpu_amd.h"', "int main(void) {"]
    for struct, cls in mirrors:
        lines.append(f'  printf("{struct} %zu\\n", sizeof({struct}));')
        for name, _ in cls._fields_:
            lines.append(f'  printf("{struct}.{name} %zu %zu\\n", offsetof({struct}, {name}), sizeof((({struct} *)0)->{name}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-I", str(HEADER.parent), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    c_side = dict(line.split(" ", 1) for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    py_side = {}
    for struct, cls in mirrors:
        py_side[struct] = str(C.sizeof(cls))
        for name, _ in cls._fields_:
            f = getattr(cls, name)
            py_side[f"{struct}.{name}"] = f"{f.offset} {f.size}"
    assert c_side == py_side
    return c_side
