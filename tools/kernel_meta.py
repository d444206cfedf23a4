"""Per-kernel resource table of a build: VGPRs, SGPRs, scratch (private segment), LDS, kernarg bytes - from the metadata notes of the code
objects in a build directory's .o files.   python tools/kernel_meta.py mhim_mil_amd/build [other/build]  (two: only the kernels that differ)

    python tools/kernel_meta.py --diff A/build B/build [--map OLD=NEW ...]
the proof step of a "no existing kernel changed" claim: the kernels present in only one of the two builds, and the kernels whose
disassembly (llvm-objdump -d without addresses and raw bytes, per symbol, end-of-function padding dropped) differs.  --map OLD=NEW (repeatable) follows a renamed kernel: the one kernel only in A whose mangled name contains OLD
and the one only in B whose name contains NEW are compared, and counted, like a kernel present in both."""
import os, re, subprocess, sys, tempfile
LLVM = "/opt/rocm/lib/llvm/bin"


def code_objects(bdir, td):
    """the gfx950 code object of every .o of a build directory, unbundled into td"""
    for f in sorted(os.listdir(bdir)):
        if not f.endswith(".o"):
            continue
        fb, co = os.path.join(td, "fb"), os.path.join(td, f + ".co")
        subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", os.path.join(bdir, f), fb], check=True)
        r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--unbundle", f"--input={fb}", f"--output={co}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], capture_output=True)
        if r.returncode == 0:
            yield co


def meta(bdir):
    txt = ""
    with tempfile.TemporaryDirectory() as td:
        for co in code_objects(bdir, td):
            txt += subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
    out = {}
    for blk in txt.split("- .agpr_count:")[1:]:
        g = lambda k: (re.search(rf"\.{k}:\s+(\S+)", blk) or [None, "?"])[1]
        name = g("name")
        out[name] = dict(vgpr=g("vgpr_count"), agpr=blk.split()[0], sgpr=g("sgpr_count"), scratch=g("private_segment_fixed_size"),
                         lds=g("group_segment_fixed_size"), kernarg=g("kernarg_segment_size"))
    return out


def disasm(bdir):
    """{kernel symbol: its instructions}; s_nop / s_code_end / elided-zero lines at the end of a function are padding up to the next one"""
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for co in code_objects(bdir, td):
            txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], capture_output=True, text=True, check=True).stdout
            for blk in re.split(r"^(?=<[^>]+>:$)", txt, flags=re.M)[1:]:
                name, _, body = blk.partition(">:\n")
                lines = [l.split("//")[0].strip() for l in body.splitlines() if l.strip()]
                while lines and lines[-1].split()[0] in ("s_nop", "s_code_end", "..."):
                    lines.pop()
                out[name[1:]] = lines
    return out


if sys.argv[1] == "--diff":
    args, maps = sys.argv[2:], []
    while "--map" in args:                                    # --map OLD=NEW: a kernel renamed between the two builds
        i = args.index("--map")
        maps.append(args[i + 1].split("=", 1))
        del args[i:i + 2]
    a, b = disasm(args[0]), disasm(args[1])
    pairs = {k: k for k in set(a) & set(b)}
    for old, new in maps:
        ka, kb = [k for k in set(a) - set(b) if old in k], [k for k in set(b) - set(a) if new in k]
        if len(ka) != 1 or len(kb) != 1:
            sys.exit(f"--map {old}={new}: needs one kernel on each side, found {ka} and {kb}")
        pairs[ka[0]] = kb[0]
        print("mapped", ka[0], "->", kb[0])
    for k in sorted(set(a) - set(pairs)):
        print("only in", args[0], k)
    for k in sorted(set(b) - set(pairs.values())):
        print("only in", args[1], k)
    changed = [k for k in sorted(pairs) if a[k] != b[pairs[k]]]
    for k in changed:
        print("differs", k, f"({len(a[k])} vs {len(b[pairs[k]])} instructions)")
    print(f"{len(pairs) - len(changed)} kernels identical, {len(changed)} differ")
    sys.exit(1 if changed else 0)
a = meta(sys.argv[1])
b = meta(sys.argv[2]) if len(sys.argv) > 2 else None
for k in sorted(a):
    if b is None:
        print(k[:70], a[k])
    elif k in b and {x: a[k][x] for x in ("vgpr", "agpr", "scratch", "lds")} != {x: b[k][x] for x in ("vgpr", "agpr", "scratch", "lds")}:
        print(k[:70], "\n   A", a[k], "\n   B", b[k])
