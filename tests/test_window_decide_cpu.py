"""The host decisions of the reader's GPU twin (linear_amd/csrc/lnr_window_hd.h: the window's size, the exit ladder of a parsed window
for each of the five sites, the advance of the BGZF chain) as a stand-alone program under the address and undefined-behaviour sanitizers.
The expected outcomes stand in tests/window_decide_main.cpp.  No GPU, nothing preloaded."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_window_decisions_under_sanitizers(tmp_path):
    exe = str(tmp_path / "window_decide_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "window_decide_main.cpp")])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("ok checks "), (p.returncode, out, p.stderr.decode()[-3000:])
    assert int(out.split()[2]) >= 90 and out.split()[4] == "0", out       # every row of the table ran
