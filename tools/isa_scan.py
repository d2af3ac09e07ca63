"""Static checks on the gfx950 ISA of the kernels (no GPU needed): the compiler pathologies of DESIGN 3.5b / 3.5c.

    python tools/isa_scan.py                 # every csrc/*.hip: kernels whose MFMAs sit behind a drain, kernels whose stores wait for each other
    python tools/isa_scan.py bf16.hip conv1d_wgrad3_bf16_kernel     # one-character-per-instruction trace of the kernels matching the name
    python tools/isa_scan.py compare DIR_A DIR_B [file.hip ...]     # two trees (a refactor and its parent): is the device code of each kernel the same?

(1) `v_mfma` with `s_waitcnt vmcnt(0|1)` among the three instructions in front of it: a weight-fragment ring that is drained every k-step
    instead of being pipelined (`a = A[p]; A[p] = load(); mfma(a)` idiom, flat accesses near the loop, prefetch values consumed at issue);
(2) basic blocks holding one or two stores behind `s_waitcnt vmcnt(0)`: `if (valid) store` per element, or load -> store -> load chains
    (vmcnt retires loads and stores in issue order on gfx9).
Trace legend: L load, S store, M MFMA, r / w LDS read / write, (vN) s_waitcnt vmcnt(N), |B| barrier, ^ branch; one line per basic block.
compare: kernels are matched by their demangled name WITHOUT template arguments (a refactor that drops a template parameter renames the
symbol); instantiations of one template pair up by the arguments that survive.  Compared: the instruction stream (no directives, no comments, no
`__hip_cuid_*`, local labels without the function index) and the register / spill / scratch / LDS entries of `.amdgpu_metadata`."""
import collections, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join(ROOT, "speech-editing-toolkit_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-S", "--cuda-device-only"]


def asm_of(src):
    out = os.path.join(tempfile.gettempdir(), "isa_scan_" + os.path.basename(src) + ".s")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        subprocess.run(["hipcc"] + FLAGS + ["-o", out, src], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read().split("\n")


def kernels(lines):
    starts = [(i, l) for i, l in enumerate(lines) if re.match(r"^_Z[A-Za-z0-9_]*:|^[a-z][a-z_0-9]*kernel[A-Za-z0-9_]*:", l)]
    for n, (i, l) in enumerate(starts):
        yield l.split(":")[0], lines[i:(starts[n + 1][0] if n + 1 < len(starts) else len(lines))]


# (3) the store-data hazard of round 5: a buffer store of more than 64 bits whose soffset is an SGPR, followed IMMEDIATELY by a
#     VALU instruction that writes one of its data registers.  ROCm 7.2 pads that pair with a wait state only when soffset is not a register;
#     on gfx950 the unpadded pair sometimes stores the overwritten dword (run-to-run differences in conv1d_mfma_v2_kernel's outputs).
WIDE_STORE = re.compile(r"(buffer_store_dwordx[34]|buffer_store_format_xyzw?|buffer_store_format_d16_xyzw) v\[(\d+):(\d+)\], "
                        r"(?:v\d+|off|v\[\d+:\d+\]), s\[\d+:\d+\], (\S+)")


def store_data_hazards(body):
    """[(store, next instruction)] pairs of one kernel body that match (3)."""
    out = []
    ins = [b.strip() for b in body if b.strip() and not b.strip().startswith((".", ";"))]
    for k, t in enumerate(ins[:-1]):
        m = WIDE_STORE.match(t)
        if not m or not re.match(r"s\d+", m.group(4)):
            continue
        lo, hi, n = int(m.group(2)), int(m.group(3)), ins[k + 1]
        if not n.startswith("v_"):
            continue
        w, wr = re.match(r"v_\w+ v(\d+)", n), re.match(r"v_\w+ v\[(\d+):(\d+)\]", n)
        if (w and lo <= int(w.group(1)) <= hi) or (wr and not (int(wr.group(2)) < lo or int(wr.group(1)) > hi)):
            out.append((t, n))
    return out


def scan(src):
    for name, body in kernels(asm_of(src)):
        nm = sum("v_mfma" in b for b in body)
        bad = sum(1 for k, b in enumerate(body) if "v_mfma" in b and re.search(r"vmcnt\((0|1)\)", " ".join(body[max(0, k - 3):k])))
        blocks, cur = [], []
        for b in body:
            t = b.strip()
            if t.startswith(".LBB") or t.startswith("; %bb."):
                blocks.append(cur); cur = []
            cur.append(t)
        blocks.append(cur)
        ser = sum(1 for blk in blocks if 1 <= sum(x.startswith(("buffer_store", "global_store", "flat_store")) for x in blk) <= 2
                  and any(re.search(r"vmcnt\(0\)", x) for x in blk))
        hz = store_data_hazards(body)
        if hz:
            print("%-18s %-90s %d wide stores with an SGPR soffset whose data registers the next VALU instruction rewrites, e.g. %s ; %s" % (
                os.path.basename(src), name[:90], len(hz), hz[0][0][:60], hz[0][1][:40]))
        if (nm and bad * 5 >= nm) or ser >= 4:
            print("%-18s %-90s MFMAs %4d, behind vmcnt(0|1): %4d | store blocks behind vmcnt(0): %d" % (os.path.basename(src), name[:90], nm, bad, ser))


def trace(src, pat):
    for name, body in kernels(asm_of(src)):
        if pat not in name:
            continue
        out = []
        for b in body:
            t = b.strip()
            if t.startswith(".LBB"): out.append("\n" + t.split(":")[0] + ":")
            elif t.startswith("v_mfma"): out.append("M")
            elif t.startswith(("buffer_load", "global_load", "flat_load")): out.append("L")
            elif t.startswith(("buffer_store", "global_store", "flat_store")): out.append("S")
            elif t.startswith("ds_read"): out.append("r")
            elif t.startswith("ds_write"): out.append("w")
            elif t.startswith("s_barrier"): out.append("|B|")
            elif t.startswith("s_waitcnt"):
                m = re.search(r"vmcnt\((\d+)\)", t)
                if m: out.append("(v%s)" % m.group(1))
            elif t.startswith(("s_cbranch", "s_branch")): out.append("^")
        s = re.sub(r"\n\.LBB\d+_\d+:\^*(?=\n|$)", "", "".join(out))
        print(name); print(s)


def tree_asm(root, f):
    root = os.path.abspath(root)
    out = os.path.join(tempfile.mkdtemp(prefix="isa_cmp_"), f + ".s")
    flags = [os.path.join(root, "include") if x == os.path.join(ROOT, "include") else x for x in FLAGS]
    subprocess.run(["hipcc"] + flags + ["-o", out, os.path.join(root, "speech-editing-toolkit_amd", "csrc", f)], check=True, stdout=subprocess.DEVNULL)
    return open(out).read().split("\n")


def strip_template_args(name):
    """('ns::k(Args)', ['true', '128']) of 'void ns::k<true, 128>(Args)' (c++filt prints the return type of template instantiations only)."""
    base, args, depth = "", "", 0
    for ch in name:
        depth -= ch == ">"
        if depth == 0:
            base += "" if ch in "<>" else ch
        else:
            args += ch
        depth += ch == "<"
        if depth == 0 and ch == ">":
            args += ","
    return re.sub(r"^void ", "", base), [a.strip() for a in args.split(",") if a.strip()]


def instructions(body):
    out = []
    for b in body[1:]:
        t = re.sub(r"\s+", " ", b.split(";")[0]).strip()
        if t.startswith(".Lfunc_end"):  # (behind it: the kernel descriptor, and after the last kernel the metadata)
            break
        if not t or "__hip_cuid_" in t or (t.startswith(".") and not re.match(r"\.LBB\d+_\d+:", t)):
            continue
        out.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


META = (".vgpr_count", ".vgpr_spill_count", ".agpr_count", ".sgpr_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def metadata(lines):
    """{symbol: {key: value}} for the keys of META, from the .amdgpu_metadata block."""
    out, cur = {}, {}
    for l in lines:
        m = re.match(r"\s+(- )?(\.[a-z_]+):\s+(\S+)\s*$", l)
        if not m:
            continue
        if m.group(1) and m.group(2) == ".agpr_count":
            cur = {}
        if m.group(2) in META:
            cur[m.group(2)] = m.group(3)
        if m.group(2) == ".name":
            out[m.group(3).strip("'")] = cur
    return out


def is_subsequence(a, b):
    it = iter(b)
    return all(x in it for x in a)


def compare(dir_a, dir_b, files):
    """Per kernel of the named csrc files: `identical`, or the first differing instructions and the opcode-count delta.  Returns the number of kernels that differ."""
    n_diff = 0
    for f in files:
        sides = []
        for root in (dir_a, dir_b):
            lines = tree_asm(root, f)
            names = [n for n, _ in kernels(lines)]
            plain = subprocess.run(["c++filt"] + names, check=True, capture_output=True, text=True).stdout.split("\n")
            meta = metadata(lines)
            sides.append([(strip_template_args(p), instructions(body), meta.get(n, {})) for (n, body), p in zip(kernels(lines), plain)])
        left = list(sides[1])
        for (base, args), ins_a, meta_a in sides[0]:
            cands = [k for k in left if k[0][0] == base]
            match = next((k for k in cands if is_subsequence(k[0][1], args) or is_subsequence(args, k[0][1])), cands[0] if cands else None)
            label = "%-18s %s <%s>" % (f, base, ", ".join(args))
            if match is None:
                print(label, "-- only in", dir_a); n_diff += 1
                continue
            left.remove(match)
            (_, args_b), ins_b, meta_b = match
            if args_b != args:
                label += " -> <%s>" % ", ".join(args_b)
            res = " ".join("%s %s" % (k[1:].replace("_count", "").replace("_fixed_size", ""), meta_a.get(k, "?")) for k in META)
            if ins_a == ins_b and meta_a == meta_b:
                print(label, "\n    identical (%d instructions; %s)" % (len(ins_a), res))
                continue
            n_diff += 1
            print(label, "\n    DIFFERENT: %d -> %d instructions" % (len(ins_a), len(ins_b)))
            for k in META:
                if meta_a.get(k) != meta_b.get(k):
                    print("    %s %s -> %s" % (k, meta_a.get(k), meta_b.get(k)))
            i = next((i for i, (x, y) in enumerate(zip(ins_a, ins_b)) if x != y), min(len(ins_a), len(ins_b)))
            for x, y in zip(ins_a[i:i + 4] + [""] * 4, (ins_b[i:i + 4] + [""] * 4)[:4]):
                print("    @%-6d %-60s | %s" % (i, x, y)); i += 1
            ca, cb = (collections.Counter(t.split()[0] for t in ins if not t.startswith(".LBB")) for ins in (ins_a, ins_b))
            print("    opcodes:", ", ".join("%s %+d" % (op, cb[op] - ca[op]) for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op]) or "same counts, another order")
        for (base, args), _, _ in left:
            print("%-18s %s <%s> -- only in %s" % (f, base, ", ".join(args), dir_b)); n_diff += 1
    return n_diff


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "compare":
        fs = sys.argv[4:] or sorted(f for f in os.listdir(CS) if f.endswith(".hip"))
        sys.exit(1 if compare(sys.argv[2], sys.argv[3], fs) else 0)
    elif len(sys.argv) >= 3:
        trace(os.path.join(CS, sys.argv[1]), sys.argv[2])
    else:
        for f in sorted(os.listdir(CS)):
            if f.endswith(".hip"):
                scan(os.path.join(CS, f))
