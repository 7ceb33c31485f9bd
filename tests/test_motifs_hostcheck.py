"""The forbidden patterns' host side under AddressSanitizer (tests/hostcheck/motifs.cpp): set / replace / clear, every refusal of the
setter with the object untouched, the note of a wild type that is not free, init / run / read on both RNG modes, both gradient
policies, two streams and next to recombination, the stateless scan, and the failure sweep over every fallible runtime call --
a stand-alone program on the mock runtime, like the other modes' drivers."""
import os
import re
import subprocess


def test_host_side_under_address_sanitizer():
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "build_and_run.sh")
    r = subprocess.run(["bash", script, "motifs", "sweep"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"hostcheck motifs ok: (\d+) fallible runtime calls per walk, (\d+) injected failures handled", r.stdout)
    assert m and int(m.group(1)) > 100 and m.group(1) == m.group(2), r.stdout
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
