"""Host: csrc/mgx_host.h (the kernel units' shared host code) as a stand-alone program on the emulated HIP runtime of
tests/cpu_emu, under AddressSanitizer + UndefinedBehaviorSanitizer: the dynamic-LDS limit is only ever raised, per device,
for every kernel of its set, also from eight threads at once; the cached MgxDev image reports a changed table and only
that.  The assertions are in tests/cpu_emu/host_header_check.cpp."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"


def test_host_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_header_check")
    emu = os.path.join(ROOT, "tests", "cpu_emu")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-DMGX_CPU_EMU", "-I", emu, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "mettagrid_amd", "csrc"), os.path.join(emu, "host_header_check.cpp"),
                    "-pthread", "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host header ok" in r.stdout, r.stdout + r.stderr
