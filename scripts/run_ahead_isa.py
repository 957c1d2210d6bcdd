"""Static count over the run-ahead loop of the lean world kernel's preset instance (csrc/mgx_world.h, mgx_world_body): how many
`s_waitcnt lgkmcnt` stand between the loop's head and its back edge.  The pipelined loop is worth what it is because an iteration
issues its seven LDS loads together and waits ONCE; that rests on an empty `asm volatile` naming the loaded values, and a compiler
that sinks the loads into their branches again brings the dependent round trips back without changing any result.  Nothing is
run on a GPU.  After a toolchain change:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I mettagrid_amd/csrc -DMGX_SLOT=0 --offload-device-only -S \
          mettagrid_amd/csrc/mgx_world_fast.hip -o world_fast.s        (several minutes)
    python scripts/run_ahead_isa.py world_fast.s

Expected (DESIGN.md "Round 11"): 1 wait on lgkmcnt, none on vmcnt, 7 ds_read, no lane moves; exit status 1 otherwise.
The loop is found as the innermost loop around the first LDS `ds_or_b32` (the dirty marks) of the instance's function."""
import re
import sys

lines = open(sys.argv[1]).read().split("\n")
start = next(i for i, l in enumerate(lines) if l.startswith("_ZN") and "mgx_world_kernel_fast_shape" in l and l.rstrip().split(":")[0].endswith("Evi"))
mark = next(i for i in range(start, len(lines)) if lines[i].lstrip().startswith("ds_or_b32"))
hdr = None
for i in range(mark, start, -1):   # the nearest block label above the marks names its loop header in a comment
    m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", lines[i])
    if m:
        hdr = m.group(1)
        break
assert hdr, "no loop around the dirty marks"
body = [i for i in range(start, len(lines)) if f"Header={hdr} " in lines[i] or lines[i].startswith(f".L{hdr}:")]
lo, hi = min(body), max(body)
while hi + 1 < len(lines) and not lines[hi + 1].startswith(".LBB"):   # the last block runs to the next label
    hi += 1
ins = [l.strip() for l in lines[lo:hi + 1] if l.startswith("\t") and not l.strip().startswith(";")]
count = lambda pat: sum(1 for l in ins if re.match(pat, l))
lgkm = sum(1 for l in ins if l.startswith("s_waitcnt") and "lgkmcnt" in l)
vm = sum(1 for l in ins if l.startswith("s_waitcnt") and "vmcnt" in l)
print(f"loop {hdr}, lines {lo + 1}-{hi + 1}: {len(ins)} instructions")
print(f"s_waitcnt lgkmcnt {lgkm}   s_waitcnt vmcnt {vm}   v_readlane/v_writelane {count(r'v_(read|write)lane')}")
print(f"ds_read {count(r'ds_read')}   ds_write {count(r'ds_write')}   ds_or {count(r'ds_or')}   stores {count(r'(flat|global)_store')}   "
      f"loads from memory {count(r'(flat|global)_load')}")
sys.exit(0 if lgkm == 1 and vm == 0 else 1)
