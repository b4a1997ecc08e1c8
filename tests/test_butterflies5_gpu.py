"""The FMA-fused 5- and 25-point butterflies of the N-point row pass (csrc/bds_acq_pfa.h: pk_radix5, pk_radix5_tw_k, pk_radix25,
pk_radix25<true>) on the device against a double-precision DFT: tools/probe/bfly5_check.hip is compiled with hipcc on the GPU box
and run -- 64 lanes x 4 random cases, the unit impulses and all-ones per form, 1e-6 of the largest output (the bound of the
16-point butterflies, tests/test_butterflies_gpu.py; fp32 rounding of a 25-point transform is ~1e-7).  The operand modifiers of
the packed instructions (op_sel / neg_lo / neg_hi) are what this checks: the compiler takes any of them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_fused_radix5_butterflies_against_double_dft(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    exe = tmp_path / "bfly5_check"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-fno-slp-vectorize", "-Wno-unused-result",
           "-I" + os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "probe", "bfly5_check.hip"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if "max |err|" in l]
    assert len(lines) == 14 and r.stdout.strip().endswith("ok"), r.stdout
    for l in lines:
        assert float(l.split("=")[-1]) < 1e-6, l
