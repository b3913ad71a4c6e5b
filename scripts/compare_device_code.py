#!/usr/bin/env python3
"""Dev tool: are the kernels of two device-only assembly files (hipcc ... --cuda-device-only -S) the same machine code?

    compare_device_code.py A.s B.s [--map OLD=NEW ...]

A kernel is the text from `.type NAME,@function` to `.end_amdhsa_kernel`: its instructions and its kernel descriptor (registers, LDS).
Comments are dropped and the per-file numbers in local labels are normalised (the function number of .LBB<n>_<m> / .Lfunc_end<n> /
.Lfunc_begin<n>; the long-branch labels .Lpost_getpc<n>, renumbered from 0 inside each kernel); kernels are compared by symbol.  --map OLD=NEW compares
A's kernel OLD with B's kernel NEW (mangled names: an instantiation whose template parameter list changed).  Exit status 1 if B has a
kernel that A lacks or a common kernel differs.
"""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, body, far = m.group(1), [], {}
        if name is None:
            continue
        line = re.sub(r"\.L(BB|func_end|func_begin)\d+", r".L\1#", line.split(";")[0]).strip()
        line = re.sub(r"\.Lpost_getpc\d+", lambda g: ".Lpost_getpc#%d" % far.setdefault(g.group(0), len(far)), line)
        if line:
            body.append(line)
        if line.startswith(".end_amdhsa_kernel"):
            out[name], name = body, None
    return out


def main(argv):
    files, maps = list(argv), []
    while "--map" in files[:-1]:
        i = files.index("--map")
        maps.append(files[i + 1])
        del files[i:i + 2]
    if len(files) != 2 or any("=" not in m for m in maps):
        sys.exit(__doc__)
    a, b = kernels(files[0]), kernels(files[1])
    for m in maps:
        old, new = m.split("=", 1)
        a[new] = [line.replace(old, new) for line in a.pop(old)]
        print(f"mapped: {old} -> {new}")
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print(f"{files[0]}: {len(a)} kernels, {files[1]}: {len(b)} kernels, {len(set(a) & set(b)) - len(differ)} identical")
    for title, names in (("only in A", only_a), ("only in B", only_b), ("differ", differ)):
        print(f"{title}: {len(names)}")
        for k in names:
            print(f"  {k}")
    return 1 if only_b or differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
