#!/usr/bin/env python3
"""Static instruction mix of every kernel in a gfx950 assembly file (hipcc ... --offload-device-only -S), for kernels whose
time is the length of one wavefront's instruction stream (the lean world kernel).  Counts are static: nothing is run.

  scripts/asm_mix.py unit.s [name filter]
"""
import re
import sys

GROUPS = (("v_readlane_b32", r"v_readlane_b32"), ("v_writelane_b32", r"v_writelane_b32"),
          ("v_mul_lo_u32 / v_mad_u64_u32", r"v_mul_lo_u32|v_mad_u64_u32"), ("v_mul_hi_u32 (division sequences)", r"v_mul_hi_u32"),
          ("vector loads", r"(global|flat|buffer|scratch)_load_\w+"), ("vector stores", r"(global|flat|buffer|scratch)_store_\w+"),
          ("s_load", r"s_load_\w+|s_buffer_load_\w+"), ("LDS", r"ds_\w+"), ("s_waitcnt", r"s_waitcnt"),
          ("branches", r"s_cbranch_\w+|s_branch"))


def main() -> int:
    want = sys.argv[2] if len(sys.argv) > 2 else ""
    text = open(sys.argv[1]).read().split("\n")
    i = 0
    while i < len(text):
        m = re.match(r"\s*\.type\s+(\S+),@function", text[i])
        if not m:
            i += 1
            continue
        name, j = m.group(1), i + 1
        while not text[j].startswith(name + ":"):
            j += 1
        k = j
        while not re.match(r"\.Lfunc_end\d+:", text[k]):
            k += 1
        i = k
        if want not in name:
            continue
        ops = [ln.split()[0] for ln in text[j + 1:k] if ln.startswith("\t") and not ln.lstrip().startswith((".", ";"))]
        print(f"{name}: {len(ops)} instructions")
        for label, pat in GROUPS:
            rx = re.compile(pat)
            print(f"  {label:36s} {sum(1 for o in ops if rx.fullmatch(o)):8d}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
