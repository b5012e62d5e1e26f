"""CPU: collect plans (per-PE byte lengths) through the p2p transport's pairing protocol,
both signalling modes, under ThreadSanitizer.

tests/p2p_proto_collect_harness.cpp reuses the backend of tests/p2p_proto_harness.cpp and
runs the product's own protocol code (sosp2p::exec_host, sosp2p::exec_stream and the
extended sosp2p::peer_sends) with the product's collect plans (sosplan::build_collect) on
CPU threads, P = 2..12: equal lengths, alternating zero and odd lengths, one long
contribution among short ones, a single contributor and all zero.  Built like
tests/test_p2p_proto.py builds its harness; a clean run means every byte a PE reads from
a peer is ordered after the peer's writes by the protocol's counters alone, every peer
read followed an acquire, every target equals the concatenation and nothing above the
sum of the lengths was written.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "build")


def test_collect_protocol_race_free():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "p2p_proto_collect_harness_tsan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "sos_amd", "csrc"),
           "-I" + os.path.join(ROOT, "tests"),
           os.path.join(ROOT, "tests", "p2p_proto_collect_harness.cpp"),
           os.path.join(ROOT, "sos_amd", "csrc", "plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([exe, "1"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"(\d+) collect calls OK .*; (\d+) peer reads, each after an acquire", r.stdout)
    # 4 modes x P in {2,3,4,5,8,12} (34 PEs) x 20 calls per PE
    assert m and int(m.group(1)) == 4 * 34 * 20 and int(m.group(2)) > 0, r.stdout
