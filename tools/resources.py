"""Registers and scratch of every render kernel in a built library (the A/B gate).

    python tools/resources.py [LIB.so | BUILD ...]        (default: the in-tree library)
    python tools/resources.py --gate BASE.so VARIANT.so   exit 1 if VARIANT spills more
    python tools/resources.py --markdown [BUILD]          DESIGN.md §3's occupancy table
    python tools/resources.py --text BASE VARIANT         exit 1 unless both (.so or .o) hold the same device
                                                          functions with the same instructions
    python tools/resources.py --census BUILD KERNEL [BEGIN [END]] [--blocks]
                                                          the kernel's instruction mix (VALU, SALU, SMEM,
                                                          branches, s_nop, v_readlane/v_writelane, ...): all
                                                          of it, and from the first instruction matching the
                                                          regular expression BEGIN to the next matching END;
                                                          --blocks: every stretch between branches

Reads the gfx950 code objects out of the library's .hip_fatbin section
(llvm-objcopy + clang-offload-bundler) and its kernel metadata notes
(llvm-readelf --notes): .vgpr_count, .sgpr_count and
.private_segment_fixed_size (scratch bytes per lane) — the numbers the
compiler's -Rpass-analysis=kernel-resource-usage remarks print (make
resource-usage), and what the occupancy follows from (512 VGPRs per SIMD
lane slot: 8 waves at <= 64, 6 at <= 80, 5 at <= 96).

rocprofv3's kernel trace reports `VGPR_Count` as half of these (32 for the
depth-0 kernel's 64, 40 for the 80 of the deep kernels): it decodes the
descriptor's granulated VGPR field with a granule of 4, where gfx950 (wave64)
allocates in granules of 8. Its scratch figure agrees with this tool.

The gate (round-4 verdict): every A/B variant's log starts with
both builds' lines for the kernels it times, and a variant whose scratch grows
at a register-capped kernel is not timed unless its prediction accounts for
the spill.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def lib_path(spec):
    if spec in ("main", None):
        return os.path.join(ROOT, "openglraytracer_amd", "libopenglraytracer_amd.so")
    if spec.endswith((".so", ".o")):
        return spec
    return os.path.join(ROOT, "_ab", spec, "libopenglraytracer_amd.so")


def kernel_name(mangled):
    """render_kernel<D, MC, DEV[, SHAPE[, LAUNCH]]> from the mangled name
    (SHAPE: the scene shapes, rt_internal.h kShapeRoom; LAUNCH: the launch
    shapes, kLaunchPlain = 1, with kLaunchPersistent 3; each left out when
    0), else the mangled name."""
    m = re.search(r"render_kernelILi(\d)ELb([01])ELb([01])E(?:Li(\d+)E)?(?:Li(\d+)E)?", mangled)
    if m:
        name = "render_kernel<%s,%s,%s" % (m.group(1), "true" if m.group(2) == "1" else "false",
                                           "true" if m.group(3) == "1" else "false")
        shape, launch = m.group(4) or "0", m.group(5) or "0"
        if shape != "0" or launch != "0":
            name += ",%s" % shape
        if launch != "0":
            name += ",%s" % launch
        return name + ">"
    m = re.search(r"animate_kernelILb([01])E", mangled)
    if m:  # the instance with the sphere phases (rt_anim.hip), or the box phases alone
        return "animate_kernel<%s>" % ("true" if m.group(1) == "1" else "false")
    if re.search(r"\d+hits_kernelE", mangled):  # the primary-hit kernel (rt_kernel.hip; not a row of the render table)
        return "hits_kernel"
    m = re.search(r"\d+aa_refine_kernelILi(\d)ELb([01])EE", mangled)  # adaptive anti-aliasing (not rows either)
    if m:  # depth, queued
        return "aa_refine_kernel<%s,%s>" % (m.group(1), "true" if m.group(2) == "1" else "false")
    if re.search(r"\d+aa_edge_kernelE", mangled):
        return "aa_edge_kernel"
    m = re.search(r"\d+rays_kernelILi(\d)EE", mangled)  # ray queries (rt_trace_rays; not rows either): depth
    if m:
        return "rays_kernel<%s>" % m.group(1)
    if re.search(r"\d+ray_hits_kernelE", mangled):
        return "ray_hits_kernel"
    if re.search(r"\d+view_rays_kernelE", mangled):
        return "view_rays_kernel"
    return mangled


def code_objects(so, d):
    """The gfx950 code objects of a library or object file, unbundled into directory d."""
    fb = os.path.join(d, "fb.bin")
    subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, so, os.path.join(d, "x")],
                   check=True, capture_output=True)
    # one bundle per translation unit with kernels, back to back in the section
    with open(fb, "rb") as f:
        data = f.read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), data)]
    for i, at in enumerate(starts):
        part, co = os.path.join(d, "fb%d.bin" % i), os.path.join(d, "k%d.co" % i)
        with open(part, "wb") as f:
            f.write(data[at:starts[i + 1] if i + 1 < len(starts) else len(data)])
        subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + part,
                        "--targets=" + TARGET, "--output=" + co], check=True, capture_output=True)
        yield co


def resources(so):
    """{kernel: {"vgpr", "sgpr", "scratch", "waves_per_simd"}} of the library's gfx950 code object."""
    with tempfile.TemporaryDirectory() as d:
        notes = "".join(subprocess.run([LLVM + "/llvm-readelf", "--notes", co], check=True, capture_output=True,
                                       text=True).stdout for co in code_objects(so, d))
    out, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(name|vgpr_count|sgpr_count|private_segment_fixed_size):\s+(\S+)", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "name":
            cur = out.setdefault(kernel_name(val), {})
        else:
            cur[{"vgpr_count": "vgpr", "sgpr_count": "sgpr", "private_segment_fixed_size": "scratch"}[key]] = int(val)
    for r in out.values():
        if "vgpr" in r:
            r["waves_per_simd"] = min(8, 512 // max(8, -(-r["vgpr"] // 8) * 8))
    return {k: v for k, v in out.items() if k.startswith(("render_kernel", "animate_kernel", "hits_kernel", "aa_", "rays_kernel", "ray_hits_kernel",
                                                         "view_rays_kernel"))}


def texts(so):
    """{symbol: its instructions} of the file's gfx950 code objects (llvm-objdump -d, without the
    addresses and encodings)."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(so, d):
            cur = None
            dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                                 check=True, capture_output=True, text=True).stdout
            for line in dis.splitlines():
                m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:$", line)
                if m:
                    cur = out.setdefault(m.group(1), [])
                elif cur is not None and line.strip() and line.strip() != "...":  # (not the padding behind a function)
                    cur.append(re.sub(r"\s*//.*$", "", line).strip())  # (the address and encoding comment)
    return out


def same_text(base, variant):
    """Prints how the two files' device functions compare; True when both have the same symbols with
    the same instruction text (their order in the code object may differ)."""
    a, b = texts(lib_path(base)), texts(lib_path(variant))
    odd = sorted(set(a) ^ set(b)) + sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print("device functions: %d and %d; on one side only or with other instructions: %d" % (len(a), len(b), len(odd)))
    for k in odd:
        print("  " + k)
    return not odd


CLASSES = ("valu", "salu", "smem", "branch", "s_nop", "lane", "lds", "vmem", "other")


def classify(ins):
    """The issue class of one disassembled instruction; "lane" (v_readlane / v_writelane, the spilled
    SGPRs' traffic) is counted beside "valu", which holds it too."""
    op = ins.split()[0]
    if op.startswith(("s_load_", "s_buffer_load_")):
        return "smem"
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_endpgm")):
        return "branch"
    if op == "s_nop":
        return "s_nop"
    if op.startswith(("s_waitcnt", "s_barrier", "s_setprio", "s_sleep", "s_sethalt", "s_trap", "s_code_end")):
        return "other"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return "valu" if op.startswith("v_") else "other"


def mix(instructions):
    n = dict.fromkeys(CLASSES, 0)
    for ins in instructions:
        n[classify(ins)] += 1
        if ins.startswith(("v_readlane", "v_writelane")):
            n["lane"] += 1
    return n


def fmt_mix(n):
    return "  ".join("%s %4d" % (k, n[k]) for k in CLASSES) + "  | all %d" % (sum(n.values()) - n["lane"])


def kernel_text(spec, kernel):
    """The instructions of the one kernel whose readable name (kernel_name) or mangled name is `kernel`."""
    found = [(k, v) for k, v in texts(lib_path(spec)).items() if kernel in (k, kernel_name(k))]
    if len(found) != 1:
        sys.exit("%s: %d kernels named %s" % (spec, len(found), kernel))
    return found[0][1]


def blocks(instructions):
    """The kernel's stretches between branches in layout order, [(first index, [instructions])]: a
    new one begins behind every branch (the disassembly carries no labels, so a branch target inside
    a stretch does not split it). Enough to find a loop's head and foot by their first instructions."""
    out, cur, at = [], [], 0
    for i, ins in enumerate(instructions):
        if not cur:
            at = i
        cur.append(ins)
        if classify(ins) == "branch":
            out.append((at, cur))
            cur = []
    if cur:
        out.append((at, cur))
    return out


def census(spec, kernel, begin=None, end=None, show_blocks=False):
    """The instruction mix of a kernel: all of it, and from the first instruction that matches the
    regular expression `begin` up to (not including) the next one behind it that matches `end` — a
    loop's head to its first useful instruction, a vote site, ... in layout order. With show_blocks,
    every stretch between branches with its first instruction, to find such anchors."""
    ins = kernel_text(spec, kernel)
    print("# %s %s" % (spec, kernel))
    print("whole kernel     " + fmt_mix(mix(ins)))
    if show_blocks:
        for at, b in blocks(ins):
            print("  @%-5d %-52s %s" % (at, b[0][:52], fmt_mix(mix(b))))
    if begin:
        lo = next((i for i, s in enumerate(ins) if re.search(begin, s)), None)
        if lo is None:
            sys.exit("no instruction matches %r" % begin)
        hi = next((i for i in range(lo + 1, len(ins)) if end and re.search(end, ins[i])), len(ins))
        print("[%d, %d)%s %s" % (lo, hi, " " * max(1, 14 - len("[%d, %d)" % (lo, hi))), fmt_mix(mix(ins[lo:hi]))))
        return mix(ins[lo:hi])
    return mix(ins)


def fmt(name, r):
    return "%-28s VGPR %3d  SGPR %3d  scratch %4d B/lane  %d waves/SIMD" % (
        name, r.get("vgpr", -1), r.get("sgpr", -1), r.get("scratch", -1), r.get("waves_per_simd", 0))


def report(spec, kernels=None):
    res = resources(lib_path(spec))
    lines = ["# resources of %s (%s)" % (spec or "main", lib_path(spec))]
    for k in sorted(res):
        if kernels is None or k in kernels:
            lines.append("#   " + fmt(k, res[k]))
    return res, "\n".join(lines)


def gate(base, variant, kernels=None):
    """Kernels whose scratch grows in `variant` against `base` (or whose
    occupancy drops): [(kernel, base, variant)]."""
    a, b = resources(lib_path(base)), resources(lib_path(variant))
    bad = []
    for k in sorted(set(a) & set(b)):
        if kernels is not None and k not in kernels:
            continue
        if b[k].get("scratch", 0) > a[k].get("scratch", 0) or b[k]["waves_per_simd"] < a[k]["waves_per_simd"]:
            bad.append((k, a[k], b[k]))
    return bad


# DESIGN.md §3's occupancy table: (row label, kernel) in the order it lists them
TABLE = [
    ("depth 0, config 2 (room, 2-B masks, > 8 views: device views, plain launch)", "render_kernel<0,false,true,18,1>"),
    ("depth 0, config 2, 49 or more 1080p views per launch (plain launch, persistent grid, the layout class's offsets)",
     "render_kernel<0,false,true,82,3>"),
    ("the same with RT_OPT_FIXED_LAYOUT 0, or a scene in the compact layout", "render_kernel<0,false,true,18,3>"),
    ("depth 0, config 2, any other launch shape", "render_kernel<0,false,true,18>"),
    ("depth 0, the shipped scene (2-B masks, 4 boxes, device views, plain launch)", "render_kernel<0,false,true,2,1>"),
    ("depth 0, Monte-Carlo, config 5", "render_kernel<0,true,false,18>"),
    ("depth 0, general", "render_kernel<0,false,false>"),
    ("depth 0, Monte-Carlo, general", "render_kernel<0,true,false>"),
    ("the primary-hit kernel (rt_render_hits, rt_pick: the general depth-0 kernel's shape, no shading)", "hits_kernel"),
    ("depth 1 (config 1)", "render_kernel<1,false,false>"),
    ("depth 2, config 3 (room, wide masks, origin lists)", "render_kernel<2,false,false,48>"),
    ("depth 2, general", "render_kernel<2,false,false>"),
    ("depth 4, config 4 (room, wide masks, origin lists)", "render_kernel<4,false,false,48>"),
    ("depth 4, general", "render_kernel<4,false,false>"),
    ("ray queries (rt_trace_rays), colours at depth 0", "rays_kernel<0>"),
    ("ray queries, depth 1", "rays_kernel<1>"),
    ("ray queries, depth 2", "rays_kernel<2>"),
    ("ray queries, depth 4", "rays_kernel<4>"),
    ("ray queries, depth 9", "rays_kernel<9>"),
    ("ray queries, the hit records (hits_kernel's body on a loaded ray)", "ray_hits_kernel"),
    ("rt_view_rays (camera_ray into the ray buffer)", "view_rays_kernel"),
    ("the animate kernel (one work-group per frame ahead of an animated render, rt_anim.hip), boxes only",
     "animate_kernel<false>"),
    ("the animate kernel with the sphere phases (scenes with moving spheres)", "animate_kernel<true>"),
]


def markdown(spec="main"):
    """The occupancy table of DESIGN.md §3, from the library's code object."""
    res = resources(lib_path(spec))
    rows = ["| kernel | VGPRs | SGPRs | waves / SIMD | scratch B / lane |", "|---|---|---|---|---|"]
    for label, k in TABLE:
        r = res.get(k)
        if r:
            rows.append("| %s: `%s` | %d | %d | %d | %d |" % (label, k, r["vgpr"], r["sgpr"], r["waves_per_simd"],
                                                            r["scratch"]))
    return "\n".join(rows)


def main():
    args = sys.argv[1:]
    if args[:1] == ["--markdown"]:
        print(markdown(args[1] if len(args) > 1 else "main"))
        return
    if args[:1] == ["--text"]:
        sys.exit(0 if same_text(args[1], args[2]) else 1)
    if args[:1] == ["--census"]:
        show = "--blocks" in args
        a = [x for x in args[1:] if x != "--blocks"]
        census(a[0], a[1], a[2] if len(a) > 2 else None, a[3] if len(a) > 3 else None, show)
        return
    if args[:1] == ["--gate"]:
        bad = gate(args[1], args[2])
        for k, x, y in bad:
            print("GATE %s: %s -> %s" % (k, fmt("", x).strip(), fmt("", y).strip()))
        sys.exit(1 if bad else 0)
    for spec in args or ["main"]:
        print(report(spec)[1])


if __name__ == "__main__":
    main()
