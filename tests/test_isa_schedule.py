"""Static guard on the compiled gfx950 ISA of the latency-critical kernels (no GPU: hipcc cross-compiles).

DESIGN 3.5b / 3.5c: the one-block-per-CU kernels that stream weight fragments from L2 through a register ring only run as designed when
the compiler keeps the ring pipelined -- round 4 found the row-split, step-boundary and layer-group kernels with `s_waitcnt vmcnt(0|1)` in
front of most MFMAs (a ring drained every k-step: B = 1 latency 60 -> 45 ms once fixed).  The fix is a pinned k-step order in the source;
this test compiles the files and fails if a later edit lets the drain come back."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("isa_scan", os.path.join(ROOT, "tools", "isa_scan.py"))
isa_scan = importlib.util.module_from_spec(spec)
spec.loader.exec_module(isa_scan)

@pytest.fixture(scope="module")
def compiled():
    """Every csrc/*.hip compiled once for gfx950 (device only, -S, resource-usage remarks), in parallel: {file: (ISA lines, remarks)}."""
    import subprocess
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    files = sorted(f for f in os.listdir(isa_scan.CS) if f.endswith(".hip"))

    def one(f):
        out = os.path.join(tempfile.gettempdir(), "isa_test_%d_%s.s" % (os.getpid(), f))
        r = subprocess.run(["hipcc"] + isa_scan.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-o", out, os.path.join(isa_scan.CS, f)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = open(out).read().split("\n")
        os.remove(out)
        return f, (lines, r.stderr)

    with ThreadPoolExecutor(max_workers=8) as ex:
        return dict(ex.map(one, files))


HOT = {  # file -> kernel-name fragments whose MFMAs must not sit behind a drained ring
    "diffnet_x3.hip": ("diffnet_stack_x3_kernel", "diffnet_stack_x3v_kernel", "diffnet_stack_split_x2_kernel"),
    "boundary.hip": ("diffnet_boundary_x2_kernel",),
    "diffnet_bf16.hip": ("diffnet_layers_t128_bf16_kernel", "diffnet_layers_reg_bf16_kernel", "diffnet_layer_fwd_bf16_kernel", "diffnet_layer_bwd_bf16_kernel"),
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
@pytest.mark.parametrize("src", sorted(HOT))
def test_weight_rings_stay_pipelined(src, compiled):
    import re
    seen = set()
    for name, body in isa_scan.kernels(compiled[src][0]):
        frag = next((f for f in HOT[src] if f in name), None)
        if frag is None:
            continue
        seen.add(frag)
        n_mfma = sum("v_mfma" in b for b in body)
        drained = sum(1 for k, b in enumerate(body) if "v_mfma" in b and re.search(r"vmcnt\((0|1)\)", " ".join(body[max(0, k - 3):k])))
        assert n_mfma >= 24, (name, n_mfma)
        # a handful of MFMAs (the first k-step of a GEMM, a loop tail: up to 12 % in the rolled loops of the layer-group kernels) legitimately
        # follow a full wait; a drained ring showed up as 45 - 70 %
        assert drained * 5 <= n_mfma, "%s: %d of %d MFMAs sit right behind s_waitcnt vmcnt(0|1)" % (name, drained, n_mfma)
    assert seen == set(HOT[src]), (seen, HOT[src])


ALLOWED_SPILLS = {  # kernels that ship with scratch; everything else must be spill-free
    "diffnet_layers_t128_bf16_kernel": 16,   # 128-frame layer groups: 10 registers, outside the GEMM loops
    "diffnet_layer_kernel": 4,               # fp32 one-launch-per-layer fallback
    "diffnet_stack_kernelILi2ELi4ELi2E": 40, # direct fp32 stack for dilation cycles the Winograd kernel does not cover
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_shipped_kernels_are_spill_free_except_the_listed_ones(compiled):
    """Round 3's review found experiment variants with 26 - 58 spilled registers compiled into the library; they are gone, and this keeps it so:
    every kernel of every csrc/*.hip is compiled for gfx950 and its `VGPRs Spill` remark checked."""
    import re
    results = [(f, v[1]) for f, v in sorted(compiled.items())]
    n_kernels, offenders = 0, []
    for f, text in results:
        cur = None
        for line in text.split("\n"):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = m.group(1)
                n_kernels += 1
            m = re.search(r"VGPRs Spill: (\d+)", line)
            if m and int(m.group(1)) > 0:
                limit = next((v for k, v in ALLOWED_SPILLS.items() if k in cur), 0)
                if int(m.group(1)) > limit:
                    offenders.append((f, cur, int(m.group(1)), limit))
    assert n_kernels > 100, n_kernels
    assert not offenders, offenders


STORE_GUARD = {  # file -> kernel-name fragments whose epilogue stores must not each wait for the previous store
    "bf16.hip": ("conv1d_bf16_kernel", "conv1x1_oneshot_bf16_kernel"),
    "conv_x2.hip": ("conv1d_x2_kernel",),
    "resblock_x2.hip": ("resblock_pair_x2_kernel",),
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
@pytest.mark.parametrize("src", sorted(STORE_GUARD))
def test_epilogue_stores_do_not_serialise(src, compiled):
    """`if (valid) buffer_store(...)` per accumulator element compiles to one basic block per element with `s_waitcnt vmcnt(0)` in each
    (the wait-count pass cannot know whether the previous block ran), and vmcnt retires stores in issue order: every store then waits
    for the one before (64 - 110 such blocks per kernel before round 4).  The epilogues mask lanes by buffer range instead."""
    import re
    seen = set()
    for name, body in isa_scan.kernels(compiled[src][0]):
        frag = next((f for f in STORE_GUARD[src] if f in name), None)
        if frag is None:
            continue
        seen.add(frag)
        blocks, cur = [], []
        for b in body:
            t = b.strip()
            if t.startswith(".LBB") or t.startswith("; %bb."):
                blocks.append(cur)
                cur = []
            cur.append(t)
        blocks.append(cur)
        ser = sum(1 for blk in blocks if 1 <= sum(x.startswith(("buffer_store", "global_store", "flat_store")) for x in blk) <= 2
                  and any(re.search(r"vmcnt\(0\)", x) for x in blk))
        assert ser <= 12, "%s: %d basic blocks hold a store behind s_waitcnt vmcnt(0)" % (name, ser)
    assert seen == set(STORE_GUARD[src]), (seen, STORE_GUARD[src])


EW_VEC4 = {  # file -> {op of an ew_kernel<4, Op> instantiation (csrc/elementwise.h): VGPRs of the hand-written _vec4 kernel it replaced}
    "train.hip": {"ConvEpilogueBwd": 19, "ActFwd": 22, "ActBwd": 26, "GateBwd": 27, "ResSkipBwd": 30},
    "glue.hip": {"AddChanMask": 20},
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
@pytest.mark.parametrize("src", sorted(EW_VEC4))
def test_elementwise_vec4_instantiations_keep_16_byte_accesses(src, compiled):
    """Both widths of an elementwise op come from one run<W>(), so the device test that compares them no longer notices a W = 4
    instantiation that the compiler lowered to four 4-byte accesses: every one must load and store dwordx4, use no scratch and stay within
    4 VGPRs of the kernel it replaced (counts of that kernel from -Rpass-analysis=kernel-resource-usage at the commit before the template)."""
    import re
    lines, remarks = compiled[src]
    usage, cur = {}, None
    for line in remarks.split("\n"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
        for key, pat in (("VGPRs", r" VGPRs: (\d+)"), ("Scratch", r" ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    seen = set()
    for name, body in isa_scan.kernels(lines):
        m = re.search(r"ew_kernelILi4ENS_\d+([A-Za-z]+?)EEE", name)
        if m is None:
            continue
        op = m.group(1)
        seen.add(op)
        text = [b.strip() for b in body]
        assert any(t.startswith(("global_load_dwordx4", "buffer_load_dwordx4")) for t in text), name
        assert any(t.startswith(("global_store_dwordx4", "buffer_store_dwordx4")) for t in text), name
        assert usage[name]["Scratch"] == 0, (name, usage[name])
        assert usage[name]["VGPRs"] <= EW_VEC4[src][op] + 4, (name, usage[name], EW_VEC4[src][op])
    assert seen == set(EW_VEC4[src]), (seen, set(EW_VEC4[src]))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_wide_store_has_its_data_registers_rewritten_by_the_next_instruction(compiled):
    """Round 5: the run-to-run differences of the fp32 training step came from
    `buffer_store_dwordx4 v[34:37], v38, s[12:15], s10 offen` immediately followed by `v_add_u32 v36, ...`: hipcc (ROCm 7.2) pads a store of
    more than 64 bits against a VALU write of its data registers only when the store's soffset is NOT an SGPR, and on gfx950 the unpadded
    pair sometimes stores the new value of the register (a few dozen of 6.5 M elements per launch, always the rewritten dword).  Measured on
    the box: that build differs in 4 of 4 repeats, `s_nop 1` behind the store / soffset 0 are bit-stable in 5 of 5.  No kernel of the library
    may contain the pattern; the reproducer build (-DSET_CONV_V2_STORE_HAZARD=1) must, so that the scan is known to see it."""
    import subprocess
    import tempfile
    n_kernels, offenders = 0, []
    for f, (lines, _) in sorted(compiled.items()):
        for name, body in isa_scan.kernels(lines):
            n_kernels += 1
            hz = isa_scan.store_data_hazards(body)
            if hz:
                offenders.append((f, name, len(hz), hz[0]))
    assert n_kernels > 100, n_kernels
    assert not offenders, offenders
    out = os.path.join(tempfile.gettempdir(), "isa_test_%d_hazard.s" % os.getpid())
    r = subprocess.run(["hipcc"] + isa_scan.FLAGS + ["-DSET_CONV_V2_STORE_HAZARD=1", "-o", out, os.path.join(isa_scan.CS, "conv1d.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(out).read().split("\n")
    os.remove(out)
    seen = sum(len(isa_scan.store_data_hazards(body)) for name, body in isa_scan.kernels(lines) if "conv1d_mfma_v2_kernel" in name)
    assert seen >= 3, "the reproducer build no longer shows the pattern (compiler changed?): the scan cannot be trusted blindly"
