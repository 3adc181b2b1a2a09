"""The hand-back feed of a shared round of tr_roadmap_solve (csrc/handback_feed.hpp) on its own: the header includes no HIP
header, so tests/cpp/handback_feed_test.cpp drives it with stubs -- plain g++, linked against nothing."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interactive-rate-tendons_amd", "csrc")


def test_handback_feed_hands_out_every_search_once_and_ends_when_the_stream_fails(tmp_path):
    exe = str(tmp_path / "handback_feed_test")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-Wall", "-Werror", "-O1", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "handback_feed_test.cpp"), "-o", exe])
    # (the time limit measures nothing: it is what turns host threads that poll a failed stream for ever into a failed test)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, timeout=60)
    assert out.returncode == 0 and "handback feed ok" in out.stdout, out.stdout
