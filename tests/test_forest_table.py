"""The table layout of the batched chains (small_gicp_amd/csrc/forest_table.hpp) on the CPU: tests/cpp/test_forest_table.cpp rebuilds
every chain's layout for 1, 2, 3 and 64 members and checks that the sections neither overlap nor leave the buffer, under the address and
undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forest_table_layouts(tmp_path):
    exe = tmp_path / "test_forest_table"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "small_gicp_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "test_forest_table.cpp"), "-o", str(exe)]
    subprocess.check_call(cmd)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.startswith("OK: 52 tables"), p.stdout
