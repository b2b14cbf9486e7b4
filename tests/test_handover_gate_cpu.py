"""The order of the two lanes' job launches (linear_amd/csrc/lnr_handover.h) as a stand-alone program under the thread sanitizer: two
threads, 10^4 batches each, random early exits and random "no round 1".  No GPU, nothing preloaded."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_handover_gate_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "handover_gate_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-o", exe, os.path.join(HERE, "handover_gate_main.cpp"), "-lpthread"])
    for seed in (1, 2):
        # (the time limit is the check that it terminates: a missed wake-up leaves a lane asleep at the gate)
        p = subprocess.run([exe, "10000", str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        out = p.stdout.decode()
        assert p.returncode == 0 and out.startswith("ok batches 10000 violations 0 "), (p.returncode, out, p.stderr.decode()[-3000:])
        f = dict(zip(out.split()[1::2], map(int, out.split()[2::2])))
        assert f["waits"] > 0 and f["early_exits"] > 0 and f["no_round1"] > 0, out      # the run met every path
