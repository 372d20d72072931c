"""CPU: build check of the lane-pair sweep's anti-Hermitian instantiations (PMODE_UNITARY_AH = 3), after
test_isa_sweep_pair.py: sweep_pair.hip is cross-compiled to assembly with the Makefile's own flags and the two instantiations the
library launches for it -- <4,0,3,512,XGLDS> with the gradient staged in LDS (the headline kernel) and in global scratch --
must have no private segment, not one scratch_ memory instruction and at most 256 VGPRs (two waves per SIMD).  The full-M
instantiations <4,0,2,512,...> stay in the library as the fallback (GRAPE_PAIR_AH=0) and for the exact gradient;
test_isa_sweep_pair.py holds those.  Skipped where there is no hipcc."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quoptimalcontrol.jl_amd", "csrc")
# template arguments <N, SAND, MODE, MAXT, XGLDS, DUMPW, VEC>
ANTIHERM_N4 = [(4, 0, 3, 512, 1, 0, 0), (4, 0, 3, 512, 0, 0, 0)]


def _hipcc():
    make_default = "/opt/rocm/bin/hipcc"
    cand = os.environ.get("HIPCC") or (make_default if os.path.exists(make_default) else shutil.which("hipcc"))
    return cand if cand and os.path.exists(cand) else None


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None or shutil.which("make") is None:
        pytest.skip("no hipcc: the ISA check needs the cross-compiler")
    flags = subprocess.check_output(["make", "-s", "-C", CSRC, "print-hipflags"], text=True).split()
    out = str(tmp_path_factory.mktemp("isa") / "sweep_pair.s")
    subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(CSRC, "sweep_pair.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    lines = open(out).read().split("\n")
    found = {}
    for i, line in enumerate(lines):
        m = re.match(r"^_ZN5grape17sweep_pair_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELb(\d)ELb(\d)EEE\w*:", line)
        if not m:
            continue
        end = next(j for j in range(i, len(lines)) if lines[j].strip().startswith("s_endpgm"))
        desc = next(j for j in range(end, len(lines)) if ".end_amdhsa_kernel" in lines[j])
        meta = {k: int(v) for k, v in re.findall(r"\.amdhsa_(private_segment_fixed_size|next_free_vgpr)\s+(\d+)",
                                                 "\n".join(lines[end:desc]))}
        body = [l.strip() for l in lines[i:end] if l.startswith("\t")]
        found[tuple(int(g) for g in m.groups())] = (meta, body)
    return found


@pytest.mark.parametrize("targs", ANTIHERM_N4, ids=[",".join(map(str, t)) for t in ANTIHERM_N4])
def test_n4_antihermitian_instantiations_have_no_private_segment(kernels, targs):
    assert targs in kernels, (targs, sorted(kernels))
    meta, body = kernels[targs]
    scratch = [l for l in body if l.startswith("scratch_")]
    print(f"sweep_pair_kernel<{targs}>: private segment {meta['private_segment_fixed_size']} B, "
          f"{meta['next_free_vgpr']} VGPRs, {len(scratch)} scratch instructions")
    assert meta["private_segment_fixed_size"] == 0, meta
    assert not scratch, scratch[:8]
    assert meta["next_free_vgpr"] <= 256, meta               # two waves per SIMD


def test_only_n4_without_the_sandwich_is_instantiated_in_the_new_mode(kernels):
    assert sorted(t for t in kernels if t[2] == 3) == sorted(ANTIHERM_N4), sorted(t for t in kernels if t[2] == 3)
