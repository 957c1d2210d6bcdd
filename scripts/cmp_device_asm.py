#!/usr/bin/env python3
"""Is the device code of a translation unit unchanged?  Compares two gfx950 assembly files function by function, whatever
the order of the functions in the file: the set of symbols, every body (kernel descriptor included) and every kernel's
metadata entry must be equal.  For host-only refactors of a unit that also holds kernels.

  F="--offload-arch=gfx950 -O3 -std=c++17 -I include -I mettagrid_amd/csrc --cuda-device-only -S"
  hipcc $F mettagrid_amd/csrc/mgx_engine.hip -o new.s        (and the same at the parent commit -> parent.s)
  scripts/cmp_device_asm.py parent.s new.s [--skip NAME ...]
--skip NAME: leave the functions whose symbol contains NAME out of the comparison (kernels the change means to touch).
"""
import re
import sys

META = (".name", ".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".kernarg_segment_size", ".max_flat_workgroup_size", ".sgpr_spill_count", ".vgpr_spill_count", ".wavefront_size")


def norm(line: str) -> str:
    """Function-local labels carry the function's ordinal in the file; comment columns shift with its width."""
    line = re.sub(r"\bBB\d+_(\d+)", r"BB#_\1", line)
    line = re.sub(r"\.L(BB|JTI|func_begin|func_end|tmp)\d+", r".L\1#", line)
    return re.sub(r"\s+", " ", line)


def parse(path: str):
    text = open(path).read().split("\n")
    bodies, meta, cur = {}, {}, {}
    i = 0
    while i < len(text):
        m = re.match(r"\s*\.type\s+(\S+),@function", text[i])
        if m:   # from the function's label to its end label: the code and, for a kernel, its .amdhsa_kernel block
            name, j = m.group(1), i + 1
            while not text[j].startswith(name + ":"):
                j += 1
            k = j
            while not re.match(r"\.Lfunc_end\d+:", text[k]):
                k += 1
            bodies[name] = [norm(x) for x in text[j:k]]
            i = k
            continue
        m = re.match(r"\s+(\.[a-z_]+):\s*(.*)$", text[i])   # amdhsa.kernels: the keys of an entry come in alphabetical order
        if m and m.group(1) in META:
            cur[m.group(1)] = m.group(2).strip()
            if m.group(1) == ".wavefront_size":
                meta[cur[".name"]] = cur
                cur = {}
        i += 1
    return bodies, meta


def main() -> int:
    args, skip, paths = sys.argv[1:], [], []
    while args:
        a = args.pop(0)
        if a == "--skip":
            skip.append(args.pop(0))
        else:
            paths.append(a)
    (b0, m0), (b1, m1) = parse(paths[0]), parse(paths[1])
    same = True
    for what, x, y in (("function bodies", b0, b1), ("kernel metadata entries", m0, m1)):
        x, y = ({k: v for k, v in t.items() if not any(n in k for n in skip)} for t in (x, y))
        diff = sorted(k for k in x if k in y and x[k] != y[k])
        print(f"{what}: {len(x)} / {len(y)}, only in the first {sorted(set(x) - set(y))}, only in the second {sorted(set(y) - set(x))}, "
              f"{len(diff)} differ {diff[:4]}")
        same = same and set(x) == set(y) and not diff
    print("IDENTICAL" if same else "DIFFERENT")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
