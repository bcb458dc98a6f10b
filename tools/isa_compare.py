#!/usr/bin/env python3
"""Compare the gfx950 machine code of every kernel of one libhskinfu.so (the base) with another (the head): each kernel
symbol of the base must exist in the head with the same instruction listing.  Prints the kernels that are missing or differ
(nothing, exit 0, when every one is identical) and the kernels only the head has.

The device code objects are taken out of the library's .hip_fatbin section (the clang offload bundles in it, the gfx950
entries; llvm-objcopy), disassembled with llvm-objdump -d and cut into functions.  Addresses, the encoding comments, the
PC-relative constants after s_getpc_b64 and the alignment padding behind a function are masked: they shift when other code
is linked in beside a kernel.  CPU only.

usage: tools/isa_compare.py BASE.so HEAD.so [--show NAME]"""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib, tmp):
    fat = os.path.join(tmp, os.path.basename(lib) + ".fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(tmp, "discard.o")])
    data = open(fat, "rb").read()
    out, pos = [], data.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + 24)
        p = pos + 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                blob = data[pos + off:pos + off + size]
                if blob[:4] != b"\x7fELF":
                    sys.exit(f"{lib}: a gfx950 entry that is not a plain ELF code object ({blob[:4]!r}): compressed bundles are not handled")
                path = os.path.join(tmp, f"{os.path.basename(lib)}.{len(out)}.co")
                open(path, "wb").write(blob)
                out.append(path)
        pos = data.find(MAGIC, pos + 24)
    return out


def kernels(lib, tmp):
    """kernel name -> normalised instruction lines"""
    funcs = {}
    for co in code_objects(lib, tmp):
        text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
        name, lines, since_getpc = None, [], 99
        for raw in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", raw)
            if m:
                if name:
                    funcs[name] = lines
                name, lines, since_getpc = m.group(1), [], 99
                continue
            if name is None or not raw.strip() or raw.startswith("Disassembly"):
                continue
            ins = re.sub(r"\s*//.*$", "", raw).strip()           # the address / encoding comment
            ins = re.sub(r"^[0-9a-f]+:\s*", "", ins)              # a leading address
            ins = re.sub(r"<[^>]*>", "<label>", ins) if "s_cbranch" not in ins and "s_branch" not in ins else ins
            since_getpc += 1
            if ins.startswith("s_getpc_b64"):
                since_getpc = 0
            elif since_getpc <= 4 and re.match(r"s_(add|addc|sub|subb)_u32", ins):
                ins = re.sub(r"0x[0-9a-f]+|-?\b\d+\b(?![\]\w])", "<pcrel>", ins)
            lines.append(ins)
        if name:
            funcs[name] = lines
    for lines in funcs.values():  # the padding behind a function (s_code_end's s_nop 0, zero fill) is not its code
        while lines and lines[-1] in ("s_nop 0", "..."):
            lines.pop()
    return funcs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("base")
    ap.add_argument("head")
    ap.add_argument("--show", help="print the differing lines of this kernel")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        base, head = kernels(a.base, tmp), kernels(a.head, tmp)
    missing = sorted(k for k in base if k not in head)
    differ = sorted(k for k in base if k in head and base[k] != head[k])
    for k in missing:
        print(f"MISSING in head: {k}")
    for k in differ:
        print(f"DIFFERS: {k} ({len(base[k])} -> {len(head[k])} instructions)")
        if a.show == k:
            import difflib
            sys.stdout.writelines(difflib.unified_diff([s + "\n" for s in base[k]], [s + "\n" for s in head[k]], "base", "head", n=1))
    added = sorted(k for k in head if k not in base)
    print(f"# {len(base)} base kernels/functions compared: {len(missing)} missing, {len(differ)} differ; new in head: "
          + (", ".join(added) if added else "none"), file=sys.stderr)
    return 1 if (missing or differ) else 0


if __name__ == "__main__":
    sys.exit(main())
