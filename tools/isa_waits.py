"""Where does hipcc put its OWN s_waitcnt vmcnt in the kernels that stage operands by LDS-DMA?

The waitcnt pass knows that `buffer_load ... lds` writes LDS and, without alias information, fences an LDS read that follows one
with s_waitcnt vmcnt(<=N) -- N = the vector-memory operations issued AFTER the last DMA, usually 0.  A software pipeline whose
look-ahead lives in counted waits (inline asm: invisible to the pass) silently loses it: in gemm256_kernel every phase's fragment
reads waited for ALL the DMAs in flight (rounds 1-5; found in round 6 by reading the ISA, not in a profile).

    python tools/isa_waits.py [file.hip ...] [--match SUBSTRING]

compiles the sources device-only to assembly and lists, per kernel with LDS-DMAs, the compiler's vmcnt waits (those outside
#ASMSTART / #ASMEND) and the instruction each one guards.  `ds_read*` right behind `vmcnt(0..1)` inside a K loop is the pattern.
lds_read_hazards() and m0_violations() check the other two ways hand-ordered LDS traffic can go wrong (tests/test_isa_waits_cpu.py).
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bridgeqa_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden",
         "-I", os.path.join(ROOT, "include"), "-I", CSRC, "--cuda-device-only", "-S"]


def kernels(asm_text):
    """{mangled name: [lines]} of every kernel of a device assembly file: everything from its label to its .Lfunc_end (blocks
    that the compiler placed behind an s_endpgm belong to the kernel too)"""
    out, name, buf = {}, None, []
    for line in asm_text.split("\n"):
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m:
            name, buf = m.group(1), []
            continue
        if name:
            if line.startswith(".Lfunc_end"):
                out[name] = buf
                name = None
            else:
                buf.append(line)
    return out


def compiler_waits(lines):
    """[(vmcnt value, mnemonic of the next instruction)] for the s_waitcnt vmcnt the COMPILER inserted (not inline asm)"""
    hits, inasm = [], False
    for i, x in enumerate(lines):
        if "#ASMSTART" in x:
            inasm = True
        if "#ASMEND" in x:
            inasm = False
        m = re.search(r"s_waitcnt vmcnt\((\d+)\)", x)
        if m and not inasm:
            nxt = [y.strip() for y in lines[i + 1:i + 4] if y.strip() and not y.strip().startswith(";")]
            hits.append((int(m.group(1)), nxt[0].split()[0] if nxt else ""))
    return hits


def lds_dmas(lines):
    return sum(1 for x in lines if "buffer_load" in x and x.rstrip().endswith("lds"))


# ---- the other two hazards of hand-ordered LDS traffic ------------------------------------------------------------------
# 1. An inline-asm ds_read returns its result as an "=v" output that has no data dependence on the separate
#    asm volatile("s_waitcnt lgkmcnt(0)") making it valid: the register allocator may legally copy or consume the value
#    before the wait.  lds_read_hazards() follows every path of the kernel's control-flow graph from such a read to an
#    s_waitcnt with lgkmcnt(0) and reports any instruction in between that reads or writes one of its destinations.
# 2. lds_dma16 (csrc/gemm_common.h) writes M0 inside its asm without declaring it: a kernel with asm LDS-DMAs must have no
#    compiler-emitted M0 access and no compiler-emitted LDS-DMA (m0_violations()).

def instructions(lines):
    """[(text, in_asm)] of a kernel body: labels ("name:") and instructions, comments, blank lines and directives dropped"""
    out, inasm = [], False
    for x in lines:
        if "#ASMSTART" in x:
            inasm = True
            continue
        if "#ASMEND" in x:
            inasm = False
            continue
        t = x.split(";")[0].strip()
        if not t:
            continue
        if t.endswith(":"):
            out.append((t, False))
        elif not t.startswith("."):
            out.append((t, inasm))
    return out


_REG = re.compile(r"\b([va])(?:(\d+)\b|\[(\d+):(\d+)\])")


def regs(text):
    """{("v"|"a", index)} named by an instruction's operands"""
    out = set()
    for m in _REG.finditer(text):
        lo = int(m.group(2) if m.group(2) is not None else m.group(3))
        hi = lo if m.group(2) is not None else int(m.group(4))
        out.update((m.group(1), r) for r in range(lo, hi + 1))
    return out


def _mnemonic(text):
    return text.split()[0]


def _blocks(insts):
    """basic blocks [(first, last + 1, successor block indices)] of an instruction list"""
    starts = {0}
    for i, (t, _) in enumerate(insts):
        if t.endswith(":"):
            starts.add(i)
        elif _mnemonic(t).startswith(("s_branch", "s_cbranch", "s_endpgm", "s_setpc")):
            starts.add(i + 1)
    starts = sorted(s for s in starts if s < len(insts))
    first_of = {insts[s][0][:-1]: b for b, s in enumerate(starts) if insts[s][0].endswith(":")}
    blocks = []
    for b, s in enumerate(starts):
        e = starts[b + 1] if b + 1 < len(starts) else len(insts)
        last = insts[e - 1][0]
        op = _mnemonic(last)
        succ = []
        if op.startswith(("s_branch", "s_cbranch")):
            tgt = last.split()[-1]
            if tgt not in first_of:
                raise ValueError("branch to an unknown label: %r" % last)
            succ.append(first_of[tgt])
        if not op.startswith(("s_branch", "s_endpgm", "s_setpc")) and b + 1 < len(starts):
            succ.append(b + 1)
        blocks.append((s, e, succ))
    return blocks


def _step(text, inasm, pending, hazards, at):
    """transfer of one instruction over the set of pending asm-read destinations"""
    if text.endswith(":"):
        return pending
    op = _mnemonic(text)
    if op == "s_waitcnt":
        return frozenset() if "lgkmcnt(0)" in text else pending
    if inasm and op.startswith("ds_read"):
        ops = text[len(op):].split(",", 1)
        dst, src = regs(ops[0]), regs(ops[1]) if len(ops) > 1 else set()
        # (its own address may be among the registers it overwrites: that is the read, not a hazard)
        hit = (dst | src) & pending
        if hit and hazards is not None:
            hazards.append((at, text, sorted(hit)))
        return pending | frozenset(dst)
    hit = regs(text) & pending
    if hit and hazards is not None:
        hazards.append((at, text, sorted(hit)))
    return pending


def lds_read_hazards(lines):
    """[(instruction index, text, [registers])]: instructions that read or write the destination of an inline-asm ds_read
    on some path before an s_waitcnt with lgkmcnt(0) (only lgkmcnt(0) counts as covering: conservative, and all the code
    uses).  Forward may-analysis over the basic blocks (labels, s_branch / s_cbranch_* and fall-through)."""
    insts = instructions(lines)
    if not insts:
        return []
    blocks = _blocks(insts)
    preds = [[] for _ in blocks]
    for b, (_, _, succ) in enumerate(blocks):
        for c in succ:
            preds[c].append(b)
    out = [frozenset() for _ in blocks]
    work = list(range(len(blocks)))
    while work:
        b = work.pop(0)
        s, e, succ = blocks[b]
        p = frozenset().union(*(out[q] for q in preds[b])) if preds[b] else frozenset()
        for i in range(s, e):
            p = _step(insts[i][0], insts[i][1], p, None, i)
        if p != out[b]:
            out[b] = p
            work.extend(c for c in succ if c not in work)
    hazards = []
    for b, (s, e, _) in enumerate(blocks):
        p = frozenset().union(*(out[q] for q in preds[b])) if preds[b] else frozenset()
        for i in range(s, e):
            p = _step(insts[i][0], insts[i][1], p, hazards, i)
    return hazards


def asm_lds_reads(lines):
    return sum(1 for t, a in instructions(lines) if a and _mnemonic(t).startswith("ds_read"))


def asm_lds_dmas(lines):
    return sum(1 for t, a in instructions(lines) if a and t.startswith("buffer_load") and t.endswith(" lds"))


def m0_violations(lines):
    """compiler-emitted instructions that touch M0 or are LDS-DMAs, in a kernel whose LDS-DMAs are inline asm ([] else)"""
    insts = instructions(lines)
    if not any(a and t.startswith("buffer_load") and t.endswith(" lds") for t, a in insts):
        return []
    return [t for t, a in insts if not a and (re.search(r"\bm0\b", t) or (t.startswith("buffer_load") and t.endswith(" lds")))]


def scan(src, defines=()):
    """{kernel: [lines]} of the device assembly of `src`, compiled with -D<d> for every d of `defines`"""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run([HIPCC] + FLAGS + ["-D" + d for d in defines] + ["-o", out, src], check=True, stderr=subprocess.DEVNULL)
        return kernels(open(out).read())


def main():
    args = sys.argv[1:]
    match = ""
    if "--match" in args:
        match = args[args.index("--match") + 1]
        args = [a for a in args if a not in ("--match", match)]
    srcs = args or [os.path.join(CSRC, f) for f in ("gemm.hip", "gemm_mid.hip", "attn.hip", "attn_persist.hip", "detbwd.hip")]
    for src in srcs:
        print("==", os.path.relpath(src, ROOT))
        for name, lines in scan(src).items():
            if match not in name or not lds_dmas(lines):
                continue
            w = [h for h in compiler_waits(lines) if h[1].startswith("ds_read")]
            print("%-100s LDS-DMAs %3d   compiler vmcnt waits in front of LDS reads: %s" % (name[:100], lds_dmas(lines), w or "none"))


if __name__ == "__main__":
    main()
