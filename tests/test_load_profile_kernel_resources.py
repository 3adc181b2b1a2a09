"""Compile-time guard for the integrators under a load profile (csrc/fk_loaded_kernel.hpp: fk_loaded_profile; csrc/fk_loaded_lin_kernel.hpp:
fk_loaded_lin_profile): the bodies of fk_loaded_uniform and fk_loaded_lin compiled once more with the stage's load row scaled by a
weight that a scalar load fetches.  At three and four tendons they are held to two waves per SIMD, the project's rule for K1's family
(TRK_K1_TWO_WAVE_MAXN), and what they spill at that budget is held to the figures of the first build.

Figures of the first build (hipcc -O3, gfx950): spilled VGPR dwords, bytes of scratch, spilled SGPRs.  Beside them the constant-load
kernels' figures from the same compile, which the shared body leaves where they were before it.

  <N, ROT, WRITE_R>    fk_loaded_profile     fk_loaded_uniform
  <3, 1, 1>            30, 124, 32           26,  84, 14
  <3, 1, 0>            52, 188,  2           38, 132,  0
  <3, 0, 1>            24, 100, 32           20,  60, 14
  <3, 0, 0>            46, 164,  4           30, 100,  0
  <4, 1, 1>            58, 212, 28           48, 172, 18
  <4, 1, 0>            70, 260,  2           58, 212,  0
  <4, 0, 1>            52, 188, 28           42, 148, 18
  <4, 0, 0>            64, 236,  2           48, 180,  0
  <8, 1, 1>            16,   0, 115           4,   0, 132      (N = 8: one wave per SIMD by launch bounds; the VGPR spills go to AGPRs,
  <8, 1, 0>            14,   0,  95           0,   0, 114       no scratch)
  <8, 0, 1>            18,   0, 113           8,   0, 132
  <8, 0, 0>            12,   0,  95           0,   0, 110

  <N, ROT>             fk_loaded_lin_profile fk_loaded_lin
  <3, 1>                0,  0,  0             4,  20,  0
  <3, 0>                0,  0,  0            10,  44,  0
  <4, 1>                2, 12,  0             2,  12,  0
  <4, 0>                0,  0,  0            26, 108,  0
  <8, 1>                0,  0, 38             0,   0, 26
  <8, 0>                0,  0, 60             0,   0, 32"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interactive-rate-tendons_amd", "csrc")

#           (N, ROT, WRITE_R): (spilled VGPR dwords, scratch bytes, spilled SGPRs)
FK_BUDGET = {(3, 1, 1): (30, 124, 32), (3, 1, 0): (52, 188, 2), (3, 0, 1): (24, 100, 32), (3, 0, 0): (46, 164, 4),
             (4, 1, 1): (58, 212, 28), (4, 1, 0): (70, 260, 2), (4, 0, 1): (52, 188, 28), (4, 0, 0): (64, 236, 2),
             (8, 1, 1): (16, 0, 115), (8, 1, 0): (14, 0, 95), (8, 0, 1): (18, 0, 113), (8, 0, 0): (12, 0, 95)}
#            (N, ROT)
LIN_BUDGET = {(3, 1): (0, 0, 0), (3, 0): (0, 0, 0), (4, 1): (2, 12, 0), (4, 0): (0, 0, 0), (8, 1): (0, 0, 38), (8, 0): (0, 0, 60)}


def _compile(tmp, name, source, extra):
    src = tmp / (name + ".hip")
    src.write_text('#include "%s"\n' % source)
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, *extra, str(src), "-o", str(tmp / (name + ".o"))],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stderr


def _figures(remarks, mangled):
    txt = remarks[remarks.index("Function Name: " + mangled):]
    get = lambda key: int(re.search(key + r"[^:]*: (\d+)", txt).group(1))
    return dict(scratch=get("ScratchSize"), vspill=get("VGPRs Spill"), sspill=get("SGPRs Spill"), occupancy=get("Occupancy"))


def _hold(f, N, budget):
    if N <= 4:
        assert f["occupancy"] >= 2
    assert f["vspill"] <= budget[0] and f["scratch"] <= budget[1] and f["sspill"] <= budget[2]


@pytest.mark.parametrize("N", [3, 4, 8])
def test_profile_integrator_keeps_its_occupancy_and_spill_budget(tmp_path, N):
    remarks = _compile(tmp_path, "prof%d" % N, "fk_inst.hip", ["-DTRK_INST_N=%d" % N, "-DTRK_INST_KIND=7"])
    assert "fk_loaded_uniform" not in remarks                    # the unit holds the profile form alone
    for rot in (1, 0):
        for wr in (1, 0):
            f = _figures(remarks, "_ZN3trk17fk_loaded_profileILi%dELb%dELb%dEEE" % (N, rot, wr))
            print("fk_loaded_profile<%d, %d, %d>: %s" % (N, rot, wr, f))
            _hold(f, N, FK_BUDGET[N, rot, wr])


@pytest.mark.parametrize("N", [3, 4, 8])
def test_profile_linearisation_keeps_its_occupancy_and_spill_budget(tmp_path, N):
    remarks = _compile(tmp_path, "plin%d" % N, "fk_lin_inst.hip", ["-DTRK_INST_N=%d" % N, "-DTRK_LIN_PROFILE"])
    assert "13fk_loaded_linILi" not in remarks
    for rot in (1, 0):
        f = _figures(remarks, "_ZN3trk21fk_loaded_lin_profileILi%dELb%dEEE" % (N, rot))
        print("fk_loaded_lin_profile<%d, %d>: %s" % (N, rot, f))
        _hold(f, N, LIN_BUDGET[N, rot])
