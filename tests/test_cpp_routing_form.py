"""The classification of a robot's routing (csrc/routing_form.hpp: table form or uniform helix, one decision per context) and the
host routing table's sign convention on their own: the header includes no HIP header, so tests/cpp/routing_form_test.cpp drives
it directly -- plain g++, linked against nothing."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interactive-rate-tendons_amd", "csrc")


def test_routing_form_classification_and_sign_convention(tmp_path):
    exe = str(tmp_path / "routing_form_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "routing_form_test.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0 and "routing form ok" in out.stdout, out.stdout
