"""CPU: build check of the lane-pair sweep's copying prologue, after test_isa_sweep_pair.py (the same `hipcc -S` recipe with the
Makefile's own flags).  The headline instantiation sweep_pair_kernel<4,0,3,512,XGLDS> copies the member's prebuilt image record
and its share of x into LDS in ONE memory round trip: ahead of the kernel's first s_barrier

  * no `s_waitcnt vmcnt` sits inside a loop (a cycle of the control-flow graph: the compiler lays predicated blocks out of line
    and jumps back from them, so a backward branch alone is no loop),
  * every global load (16 passes over x, 4 over the record, the norm bound) is issued before the first such wait,
  * and there is at most one barrier before phase A -- before the first FP64 arithmetic instruction: the copying prologue has
    none, phase A starts with the generator's FMAs;

and the kernel needs no more registers than before the record existed: 233 VGPRs, no private segment.  The building prologue
lives on in sweep_pair_build_kernel (GRAPE_PAIR_IMAGE=0 and the shapes beyond the copy's register batch): its n = 4 unitary
instantiations keep what test_isa_sweep_pair.py / test_isa_sweep_pair_antiherm.py ask of the copying ones.  Skipped where there
is no hipcc."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quoptimalcontrol.jl_amd", "csrc")
HEADLINE = (4, 0, 3, 512, 1, 0, 0)                            # <N, SAND, MODE, MAXT, XGLDS, DUMPW, VEC>
PARENT_VGPRS = 233                                            # the headline instantiation with the building prologue
# (XGLDS only: with x and the gradient in global scratch sweep_pair_kernel itself keeps the building prologue)
UNITARY_N4 = [(4, 0, 3, 512, 1, 0, 0), (4, 0, 2, 512, 1, 0, 0), (4, 0, 2, 512, 1, 1, 0), (4, 1, 2, 512, 1, 0, 0)]
X_PASSES, RECORD_PASSES = 16, 4                               # kPairXBatch, kPairImgBatch of sweep_pair.hip


def _hipcc():
    make_default = "/opt/rocm/bin/hipcc"
    cand = os.environ.get("HIPCC") or (make_default if os.path.exists(make_default) else shutil.which("hipcc"))
    return cand if cand and os.path.exists(cand) else None


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{(kernel name, template arguments): (descriptor figures, instruction and label lines)}"""
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
        m = re.match(r"^_ZN5grape\d+(sweep_pair_kernel|sweep_pair_build_kernel)ILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELb(\d)ELb(\d)EEE\w*:", line)
        if not m:
            continue
        end = next(j for j in range(i, len(lines)) if lines[j].strip().startswith("s_endpgm"))
        desc = next(j for j in range(end, len(lines)) if ".end_amdhsa_kernel" in lines[j])
        meta = {k: int(v) for k, v in re.findall(r"\.amdhsa_(private_segment_fixed_size|next_free_vgpr)\s+(\d+)",
                                                 "\n".join(lines[end:desc]))}
        body = [l.rstrip() for l in lines[i + 1:end + 1] if l.startswith("\t") or re.match(r"^\.LBB\d+_\d+:", l)]
        body = [l for l in body if l.startswith(".LBB") or not l.strip().startswith((";", "."))]
        found[(m.group(1), tuple(int(g) for g in m.groups()[1:]))] = (meta, body)
    return found


def _blocks_in_cycles(body):
    """the control-flow graph of a kernel's text: [(first line, last line)] of the basic blocks that lie on a cycle"""
    starts = {0}
    label_at = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            label_at[m.group(1)] = i
            starts.add(i)
        elif re.match(r"\s+s_c?branch", l) or l.strip().startswith("s_endpgm"):
            starts.add(i + 1)
    starts = sorted(s for s in starts if s < len(body))
    block_of = {}
    spans = []
    for b, s in enumerate(starts):
        e = (starts[b + 1] if b + 1 < len(starts) else len(body)) - 1
        spans.append((s, e))
        for i in range(s, e + 1):
            block_of[i] = b
    succ = []
    for b, (s, e) in enumerate(spans):
        out = []
        last = body[e].strip()
        m = re.match(r"s_(c?)branch\w*\s+(\.LBB\d+_\d+)", last)
        if m:
            out.append(block_of[label_at[m.group(2)]])
        if not (last.startswith("s_endpgm") or (m and not m.group(1))) and b + 1 < len(spans):
            out.append(b + 1)                                 # falls through
        succ.append(out)
    cyc = set()
    for b in range(len(spans)):                               # on a cycle: reachable from one of its own successors
        seen, work = set(), list(succ[b])
        while work:
            v = work.pop()
            if v == b:
                cyc.add(b)
                break
            if v not in seen:
                seen.add(v)
                work.extend(succ[v])
    return [spans[b] for b in sorted(cyc)]


def _is_vm_wait(l):
    return "s_waitcnt" in l and "vmcnt" in l


def test_headline_prologue_is_one_round_trip(kernels):
    meta, body = kernels[("sweep_pair_kernel", HEADLINE)]
    bar = next(i for i, l in enumerate(body) if l.strip().startswith("s_barrier"))
    looped = [(s, e) for s, e in _blocks_in_cycles(body) if s < bar]
    in_loop = [body[i].strip() for s, e in looped for i in range(s, min(e, bar) + 1) if _is_vm_wait(body[i])]
    loads = [i for i in range(bar) if re.match(r"\s+global_load", body[i])]
    waits = [i for i in range(bar) if _is_vm_wait(body[i])]
    fp64 = next(i for i, l in enumerate(body) if re.match(r"\s+v_(fma|mul|add)_f64", l))
    barriers = [i for i in range(fp64) if body[i].strip().startswith("s_barrier")]
    print(f"headline: first s_barrier at line {bar}, {len(loads)} global loads and {len(waits)} vmcnt waits ahead of it, "
          f"{len(looped)} blocks on cycles there, first FP64 instruction at line {fp64}, {len(barriers)} barrier(s) before it")
    assert not in_loop, in_loop
    assert len(loads) >= X_PASSES + RECORD_PASSES + 1, len(loads)
    assert waits and loads[-1] < waits[0], (loads[-1], waits[0])     # every load is in flight before the first wait
    assert len(barriers) <= 1, barriers


def test_headline_registers_do_not_grow(kernels):
    meta, body = kernels[("sweep_pair_kernel", HEADLINE)]
    scratch = [l for l in body if l.strip().startswith("scratch_")]
    print(f"headline: {meta['next_free_vgpr']} VGPRs, private segment {meta['private_segment_fixed_size']} B")
    assert meta["private_segment_fixed_size"] == 0 and not scratch, (meta, scratch[:8])
    assert meta["next_free_vgpr"] <= PARENT_VGPRS, meta


@pytest.mark.parametrize("targs", UNITARY_N4, ids=[",".join(map(str, t)) for t in UNITARY_N4])
def test_building_prologue_instantiations_keep_two_waves_per_simd(kernels, targs):
    assert ("sweep_pair_build_kernel", targs) in kernels, sorted(kernels)
    meta, body = kernels[("sweep_pair_build_kernel", targs)]
    scratch = [l for l in body if l.strip().startswith("scratch_")]
    assert meta["private_segment_fixed_size"] == 0 and not scratch, (meta, scratch[:8])
    assert meta["next_free_vgpr"] <= 256, meta
