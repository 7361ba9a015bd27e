"""Scalar-register spill traffic of every k_step instantiation, counted in the compiler's assembly (device-only compile, no GPU needed).

The register allocator parks scalar registers it cannot keep in lanes of a VGPR ("SGPR spill to VGPR lane"): a v_writelane_b32 where
the value is parked, a v_readlane_b32 -- usually followed by a hazard s_nop -- wherever it is used.  kernel_resources.py shows how many
registers are parked (spillS); this tool shows WHERE the traffic sits, per kernel:
  kernel    the whole kernel;
  pre-loop  everything in front of the sub-step loop's header (record load, derive(), the step-begin hooks);
  loop head the run of top-level blocks from the loop's header to its first nested loop, in layout order: where the compiler lays the
            fall-through code of the fused phases (with a few cold blocks in between);
  loop top  the sub-step loop's top-level blocks: the blocks whose innermost loop is the sub-step loop itself -- the two fused phases
            of the quiet path (substep_phase1 / substep_phase2 and what they inline) and the branch code around the rare paths; the
            contact loops (resolve passes, push, undo, snapshot) are nested loops and are NOT counted here.
The sub-step loop is found through the compiler's own comments ("=>This Loop Header: Depth=1", "in Loop: Header=BBx_y Depth=1",
"Parent Loop BBx_y Depth=1"): the Depth=1 loop with the most instructions in it, nested loops included; in rr_rollout's kernels
(MULTI) the loop over the steps is Depth=1, so there the largest Depth=2 loop.
It counts the three mnemonics v_readlane_b32, v_writelane_b32, s_nop (and instructions) and nothing else.

usage: python tools/loop_spill_traffic.py [filter-substring] [--asm=FILE] [--keep-asm=FILE] [--remarks-out=FILE] [extra hipcc flags...]
  --asm=FILE          analyse an assembly file that is already there instead of compiling (about two minutes)
  --keep-asm=FILE     where to leave the assembly of this compile (default: a temporary file, removed)
  --remarks-out=FILE  also keep hipcc's resource remarks of this compile, for kernel_resources.py --remarks=FILE
The compile is the tuning configuration (-DRR_CFG_SUBSET: T and G in fp64; -DRR_TUNE_VW_D=4 adds D)."""
import os, re, subprocess, sys, tempfile
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "roborugby_amd", "csrc", "rr_kernels.hip")
COUNTED = ("v_readlane_b32", "v_writelane_b32", "s_nop")


def opt(name):
    v = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith(name + "=")]
    return v[0] if v else None


OWN = ("--asm", "--keep-asm", "--remarks-out")
flt = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else ""
extra = [a for a in sys.argv[1:] if a.startswith("-") and a.split("=", 1)[0] not in OWN]


def assembly():
    if opt("--asm"):
        return open(opt("--asm")).read()
    keep = opt("--keep-asm")
    path = keep
    if not path:
        fd, path = tempfile.mkstemp(suffix=".s")
        os.close(fd)
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "--offload-device-only", "-S",
           "-DRR_CFG_SUBSET", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", path] + extra
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode:
        sys.exit(p.stderr[-4000:])
    if opt("--remarks-out"):
        open(opt("--remarks-out"), "w").write(p.stderr)
    text = open(path).read()
    if not keep:
        os.remove(path)
    return text


class Block:
    def __init__(self, label):
        self.label, self.inner, self.parents, self.header_depth = label, None, [], 0  # innermost loop (header label, depth), enclosing loops
        self.n = 0
        self.c = dict.fromkeys(COUNTED, 0)

    def loops(self):  # every loop the block is in: (header label, depth)
        own = [(self.label, self.header_depth)] if self.header_depth else []
        return own + ([self.inner] if self.inner else []) + self.parents


def blocks_of(lines):
    """the kernel's basic blocks in layout order, each with its loop annotations and counts"""
    out = [Block("entry")]
    for ln in lines:
        m = re.match(r"(?:\.L(BB\d+_\d+):|; %bb\.(\d+):)(.*)", ln)
        if m:
            out.append(Block(m.group(1) or "bb." + m.group(2)))
            ln = m.group(3)
        b = out[-1]
        if ln.lstrip().startswith(";"):  # a comment line, or the comment behind a label: the loop annotations
            c = ln
            m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", c)
            if m: b.inner = (m.group(1), int(m.group(2)))
            m = re.search(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", c)
            if m: b.parents.append((m.group(1), int(m.group(2))))
            m = re.search(r"=>\s*This (?:Inner )?Loop Header: Depth=(\d+)", c)
            if m: b.header_depth = int(m.group(1))
            continue
        m = re.match(r"\s+([a-z_0-9]+)", ln)
        if m and not ln.lstrip().startswith("."):
            b.n += 1
            if m.group(1) in COUNTED: b.c[m.group(1)] += 1
    return out


def total(blocks):
    return [sum(b.n for b in blocks)] + [sum(b.c[k] for b in blocks) for k in COUNTED]


def tag_of(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    m = re.match(r"void k_step<rr::Cfg<(\d+), (\d+), (\d+), (\d+), (\w+), (\d+)>, (\w+), (\w+), (\w+)>", name)
    return (name[:60], False) if not m else ("k_step %s+%s/%s+%s %s VW%s out=%s multi=%s budget=%s" % m.groups(), m.group(8) == "true")


def main():
    lines = assembly().splitlines()
    print("%-58s %-9s %7s %9s %10s %6s" % ("kernel", "where", "instrs", "readlane", "writelane", "s_nop"))
    i = 0
    while i < len(lines):
        m = re.match(r"(_Z\w*6k_stepI\w+):", lines[i])
        if not m:
            i += 1; continue
        j = i + 1
        while not lines[j].startswith(".Lfunc_end"): j += 1
        tag, multi = tag_of(m.group(1))
        body, i = lines[i + 1:j], j
        if flt and flt not in tag: continue
        bl = blocks_of(body)
        depth = 2 if multi else 1
        above = {b.label: b.parents for b in bl if b.header_depth}  # only a loop's header names the loops around it
        size = {}
        for b in bl:
            for lp in set(b.loops() + (above.get(b.inner[0], []) if b.inner else [])):
                if lp[1] == depth: size[lp[0]] = size.get(lp[0], 0) + b.n
        head = max(size, key=size.get)  # the sub-step loop's header label
        at = next(k for k, b in enumerate(bl) if b.label == head)
        top = [b for b in bl if (b.label == head and b.header_depth) or b.inner == (head, depth)]
        end = next((k for k in range(at + 1, len(bl)) if any(lp[1] > depth for lp in bl[k].loops())), len(bl))
        head_run = [b for b in bl[at:end] if b in top]
        for where, part in (("kernel", bl), ("pre-loop", bl[:at]), ("loop head", head_run), ("loop top", top)):
            print("%-58s %-9s %7d %9d %10d %6d" % ((tag, where) + tuple(total(part))))
        print("%-58s %-9s %s, %d instructions in the loop with its nested loops" % ("", "", head, size[head]))


main()
