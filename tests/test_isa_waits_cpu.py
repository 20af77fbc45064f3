"""The kernels that stage operands by LDS-DMA keep their look-ahead: hipcc must not fence the tile loop's LDS reads with its own
s_waitcnt vmcnt (tools/isa_waits.py).  Round 6 found vmcnt(0) in front of every phase's fragment reads of gemm256_kernel -- the
kernel's counted waits were decoration -- and the same fence in the contraction-major forms of gemm128 / gemm64, in wgrad_rows
and on every LDS access of sa_bwd; the reads (or the DMAs) are inline asm since.  Compiles three sources device-only to
assembly (~15 s each)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
@pytest.mark.parametrize("src,families,at_least", [("gemm.hip", ("gemm256_kernel", "gemm64_kernel", "wgrad_rows_kernel", "pwconv64"), 40),
                                                   ("gemm_mid.hip", ("gemm128_kernel",), 10),
                                                   ("detbwd.hip", ("sa_bwd_kernel",), 20)])
def test_tile_loops_have_no_compiler_fence_in_front_of_their_lds_reads(src, families, at_least):
    import isa_waits
    ks = isa_waits.scan(os.path.join(ROOT, "bridgeqa_amd", "csrc", src))
    seen = 0
    for name, lines in ks.items():
        if not any(f in name for f in families) or not isa_waits.lds_dmas(lines):
            continue
        mf = [i for i, x in enumerate(lines) if "v_mfma" in x]
        if not mf:
            continue
        seen += 1
        # the tile loop = everything up to the last v_mfma (epilogues read their output images back with compiler-visible loads)
        bad = [h for h in isa_waits.compiler_waits(lines[:mf[-1]]) if h[1].startswith("ds_read")]
        assert not bad, (name, bad)
    assert seen >= at_least, seen


# ---- the fenced build, the asm-read hazard and M0 (tools/isa_waits.py) --------------------------------------------------
FENCED = ("BQ_G256_ASM_READS=0", "BQ_DMA_ASM=0", "BQ_CF_ASM_READS=0")   # = tests/test_lds_pipeline_gpu.py's oracle build
FAMILIES = {"gemm.hip": ("gemm256_kernel", "gemm64_kernel", "wgrad_rows_kernel", "pwconv64"),
            "gemm_mid.hip": ("gemm128_kernel",), "detbwd.hip": ("sa_bwd_kernel",)}
_ASM = {}


def _asm(src, defines=()):
    import isa_waits
    key = (src, defines)
    if key not in _ASM:
        _ASM[key] = isa_waits.scan(os.path.join(ROOT, "bridgeqa_amd", "csrc", src), defines)
    return _ASM[key]


def _tile_loop(lines):
    mf = [i for i, x in enumerate(lines) if "v_mfma" in x]
    return lines[:mf[-1]] if mf else []


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
@pytest.mark.parametrize("src", sorted(FAMILIES))
def test_fenced_build_orders_lds_traffic_by_the_compiler(src):
    """The oracle build of the GPU comparison really is the compiler-ordered code: no inline-asm fragment read or LDS-DMA is
    left in any tile loop, every loop with transposed reads carries the compiler's own vmcnt fence, and every family whose
    default build orders LDS traffic by hand (pwconv64 has none: its reads and DMAs are compiler-visible in both builds) shows
    such fences -- else the comparison would hold a build against itself."""
    import isa_waits
    default, fenced = _asm(src), _asm(src, FENCED)
    assert set(default) == set(fenced)
    for fam in FAMILIES[src]:
        names = [n for n in fenced if fam in n and isa_waits.lds_dmas(fenced[n]) and _tile_loop(fenced[n])]
        assert names, fam
        hand, fenced_seen = 0, 0
        for n in names:
            loop = _tile_loop(fenced[n])
            assert isa_waits.asm_lds_reads(loop) == 0 and isa_waits.asm_lds_dmas(fenced[n]) == 0, n
            fence = [h for h in isa_waits.compiler_waits(loop) if h[1].startswith("ds_read")]
            if any("ds_read_b64_tr" in x for x in loop):
                assert fence, n
            fenced_seen += bool(fence)
            hand += bool(isa_waits.asm_lds_reads(_tile_loop(default[n])) or isa_waits.asm_lds_dmas(default[n]))
        if fam == "pwconv64":
            assert hand == 0, "pwconv64 orders LDS traffic by hand now: its fenced build must show compiler fences"
        else:
            assert hand and fenced_seen, (fam, hand, fenced_seen)


# every csrc source with kernels whose fragment reads or LDS-DMAs are inline asm, and the least number of such kernels
ASM_LDS = {"gemm.hip": (31, 12), "gemm_mid.hip": (12, 0), "detbwd.hip": (0, 44)}


def test_every_source_with_asm_lds_traffic_is_scanned():
    import re
    csrc = os.path.join(ROOT, "bridgeqa_amd", "csrc")
    asm_hdrs = set()
    users = set()
    for f in sorted(os.listdir(csrc)):
        text = open(os.path.join(csrc, f)).read()
        has = re.search(r'asm\s+volatile\s*\(\s*"[^"]*(ds_read|buffer_load[^"]*lds)', text) is not None
        if has and f.endswith(".h"):
            asm_hdrs.add(f)
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(".hip"):
            continue
        text = open(os.path.join(csrc, f)).read()
        if re.search(r'asm\s+volatile\s*\(\s*"[^"]*(ds_read|buffer_load[^"]*lds)', text) or \
                any('#include "%s"' % h in text for h in asm_hdrs):
            users.add(f)
    assert users == set(ASM_LDS), users


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
@pytest.mark.parametrize("src", sorted(ASM_LDS))
def test_asm_fragment_reads_are_untouched_until_their_wait_and_m0_is_the_asm_dmas_own(src):
    """(1) No instruction reads or writes the destination of an inline-asm ds_read before an s_waitcnt lgkmcnt(0) on any path
    of the kernel's control-flow graph: the "=v" outputs have no data dependence on the separate wait asm that makes them
    valid.  (2) A kernel with inline-asm LDS-DMAs (lds_dma16: writes M0 undeclared) has no compiler-emitted M0 access and no
    compiler-emitted LDS-DMA."""
    import isa_waits
    reads, dmas = 0, 0
    for name, lines in _asm(src).items():
        hz = isa_waits.lds_read_hazards(lines)
        assert not hz, (name, hz[:4])
        m0 = isa_waits.m0_violations(lines)
        assert not m0, (name, m0[:4])
        reads += isa_waits.asm_lds_reads(lines) > 0
        dmas += isa_waits.asm_lds_dmas(lines) > 0
    at_least_reads, at_least_dmas = ASM_LDS[src]
    assert reads >= at_least_reads and dmas >= at_least_dmas, (reads, dmas)


def _k(body):
    return ("\t" + body.strip().replace("\n", "\n\t")).split("\n") + ["\ts_endpgm"]


ASM_READ = ";;#ASMSTART\nds_read_b128 v[4:7], v2\n;;#ASMEND"
WAIT = ";;#ASMSTART\ns_waitcnt lgkmcnt(0)\n;;#ASMEND"


def test_hazard_checker_reports_what_it_exists_to_catch():
    import isa_waits
    # a copy of a pending destination on the fall-through path
    hz = isa_waits.lds_read_hazards(_k(ASM_READ + "\ns_cmp_eq_u32 s0, 0\ns_cbranch_scc1 .LBB0_2\nv_mov_b32_e32 v9, v5\n"
                                       + WAIT + "\n.LBB0_2:\n" + WAIT))
    assert [h[1] for h in hz] == ["v_mov_b32_e32 v9, v5"]
    # an MFMA reading one at a branch target whose path skips the wait (the fall-through path waits)
    hz = isa_waits.lds_read_hazards(_k(ASM_READ + "\ns_cbranch_vccnz .LBB0_2\n" + WAIT + "\n.LBB0_2:\n"
                                       "v_mfma_f32_16x16x32_bf16 a[0:3], v[4:7], v[8:11], a[0:3]"))
    assert [h[1] for h in hz] == ["v_mfma_f32_16x16x32_bf16 a[0:3], v[4:7], v[8:11], a[0:3]"]
    # a later asm read using a pending destination as its address, and one overwriting a pending destination
    hz = isa_waits.lds_read_hazards(_k(ASM_READ + "\n;;#ASMSTART\nds_read_b64_tr_b16 v[10:11], v6\n;;#ASMEND\n" + WAIT))
    assert len(hz) == 1 and "v[10:11], v6" in hz[0][1]
    hz = isa_waits.lds_read_hazards(_k(ASM_READ + "\n;;#ASMSTART\nds_read_b64_tr_b16 v[7:8], v3\n;;#ASMEND\n" + WAIT))
    assert len(hz) == 1
    # a loop whose back edge carries a pending read into its head
    hz = isa_waits.lds_read_hazards(_k(".LBB0_1:\nv_add_u32_e32 v1, v4, v1\n" + ASM_READ + "\ns_cbranch_scc0 .LBB0_1\n" + WAIT))
    assert "v_add_u32_e32 v1, v4, v1" in [h[1] for h in hz]


def test_hazard_checker_passes_clean_code():
    import isa_waits
    clean = _k("v_add_u32_e32 v6, 64, v6\n;;#ASMSTART\nds_read_b64_tr_b16 v[164:165], v166\n;;#ASMEND\n"
               ";;#ASMSTART\nds_read_b128 v[4:7], v4 offset:512\n;;#ASMEND\n"
               "v_mov_b32_e32 v9, v1 ; v4 in a comment\ns_cbranch_scc1 .LBB0_2\n" + WAIT + "\ns_branch .LBB0_3\n"
               ".LBB0_2:\ns_waitcnt vmcnt(0) lgkmcnt(0)\n.LBB0_3:\n"
               "v_mfma_f32_16x16x32_bf16 a[0:3], v[4:7], v[164:167], a[0:3]")
    assert isa_waits.asm_lds_reads(clean) == 2
    assert isa_waits.lds_read_hazards(clean) == []
    # lgkmcnt(1) does not count as covering
    assert isa_waits.lds_read_hazards(_k(ASM_READ + "\ns_waitcnt lgkmcnt(1)\nv_mov_b32_e32 v0, v4"))


def test_m0_checker():
    import isa_waits
    dma = ";;#ASMSTART\ns_mov_b32 m0, s4\ns_nop 0\nbuffer_load_dwordx4 v1, s[8:11], 0 offen lds\n;;#ASMEND"
    assert isa_waits.m0_violations(_k(dma + "\nv_mov_b32_e32 v0, v1")) == []
    assert isa_waits.m0_violations(_k(dma + "\ns_mov_b32 m0, s5")) == ["s_mov_b32 m0, s5"]
    assert isa_waits.m0_violations(_k(dma + "\nbuffer_load_dwordx4 v1, s[8:11], 0 offen lds")) != []
    # a kernel whose DMAs are all compiler-emitted may use M0 as it likes
    assert isa_waits.m0_violations(_k("s_mov_b32 m0, s5\nbuffer_load_dwordx4 v1, s[8:11], 0 offen lds")) == []
