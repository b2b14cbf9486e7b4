"""CPU: the one store routine of the GPU writer (span_store / span_copy / span_fill, linear_amd/csrc/lnr_span_hd.h: destination-aligned
dwords, single bytes at the two edges) as a stand-alone program (tests/output_span_main.cpp) under the address and undefined-behaviour
sanitizers: every destination and source misalignment, the lengths around the dword, the 256-byte and the window size, a wave and a
workgroup of lanes.  The program checks the bytes and the guards around them; the sanitizers check that nothing outside the destination
is written and nothing outside the source and its documented slack is read."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_span_under_sanitizers(tmp_path):
    exe = str(tmp_path / "output_span_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "output_span_main.cpp")])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    # 2 team sizes x 30 lengths x 4 destination misalignments x (1 fill + 4 source misalignments)
    assert p.stdout.decode().strip() == "ok 1200"
