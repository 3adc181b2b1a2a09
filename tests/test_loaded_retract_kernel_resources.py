"""Compile-time guard for the loaded FK kernels of retraction robots (csrc/fk_loaded_retract_kernel.hpp, kind 8 of csrc/fk_inst.hip): every
instantiation for 1 .. 8 tendons compiles for gfx950, and the occupancy the compiler reports is at least what the kernel's
__launch_bounds__ declare -- two waves per SIMD up to TRK_LR_TWO_WAVE_MAXN tendons, one beyond (the split of the unloaded retraction
kernel; the header says what it rests on).  The scratch sizes are printed, not asserted: nobody has measured what they cost, and
DESIGN.md records them beside the split."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interactive-rate-tendons_amd", "csrc")
KIND = 8


def _two_wave_maxn():
    """TRK_LR_TWO_WAVE_MAXN as the headers define it: TRK_K1R_TWO_WAVE_MAXN's value unless it has one of its own."""
    text = open(os.path.join(CSRC, "fk_loaded_retract_kernel.hpp")).read()
    m = re.search(r"#define TRK_LR_TWO_WAVE_MAXN (\w+)", text)
    if m.group(1).isdigit():
        return int(m.group(1))
    text = open(os.path.join(CSRC, "fk_retract_kernel.hpp")).read()
    return int(re.search(r"#define %s (\d+)" % m.group(1), text).group(1))


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    """n_tendons -> [(kernel name, {figure: value})] from -Rpass-analysis=kernel-resource-usage; the eight compilations run side by side"""
    d = tmp_path_factory.mktemp("lret")
    procs = {n: subprocess.Popen(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only",
                                  "-Rpass-analysis=kernel-resource-usage", "-DTRK_INST_N=%d" % n, "-DTRK_INST_KIND=%d" % KIND,
                                  os.path.join(CSRC, "fk_inst.hip"), "-o", str(d / ("m%d.o" % n))],
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for n in range(1, 9)}
    out = {}
    for n, p in procs.items():
        _, err = p.communicate()
        assert p.returncode == 0, err[-2000:]
        out[n] = [(name, {k.strip(): int(v) for k, v in re.findall(r"remark:\s+([A-Za-z /\[\]]+?)(?: \[[^\]]*\])?: (\d+)", body)})
                  for name, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", err, re.S)]
    return out


@pytest.mark.parametrize("n", range(1, 9))
def test_every_instantiation_compiles_at_its_declared_occupancy(remarks, n):
    kernels = remarks[n]
    fk = [(k, f) for k, f in kernels if "fk_loaded_retract" in k]
    start = [(k, f) for k, f in kernels if "shoot_start_retract" in k]
    assert len(fk) == 4 and len(start) == 1, [k for k, _ in kernels]          # ROT x WRITE_R, and the start kernel
    want = 2 if n <= _two_wave_maxn() else 1
    for k, f in fk + start:
        print("N=%d %s: occupancy %d, VGPRs %d, scratch %d B/lane, VGPR spills %d, SGPR spills %d"
              % (n, re.sub(r"^_ZN3trk\d+", "", k)[:28], f["Occupancy"], f["VGPRs"], f["ScratchSize"], f["VGPRs Spill"], f["SGPRs Spill"]))
    for k, f in fk:
        assert f["Occupancy"] >= want, (k, f)
    for k, f in start:                                   # __launch_bounds__(64): one wave per SIMD is all it declares
        assert f["Occupancy"] >= 1, (k, f)
