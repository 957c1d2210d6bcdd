"""Host: csrc/mgx_agent_rules.h (the per-agent rules of the world kernels: orientation table, footprint, result / resolved /
outcome bytes, handle_action's bookkeeping in its LDS-side, integer and stat-row forms, track_coverage) as a stand-alone
program on the emulated HIP runtime of tests/cpu_emu, under AddressSanitizer + UndefinedBehaviorSanitizer.  Exhaustive over
the rules' small domains; the assertions are in tests/cpu_emu/agent_rules_check.cpp."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"


def test_agent_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "agent_rules_check")
    emu = os.path.join(ROOT, "tests", "cpu_emu")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-DMGX_CPU_EMU", "-I", emu, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "mettagrid_amd", "csrc"), os.path.join(emu, "agent_rules_check.cpp"),
                    "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "agent rules ok" in r.stdout, r.stdout + r.stderr
