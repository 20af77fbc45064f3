"""The deterministic training mode without a GPU: its switch (bridgeqa_amd.set_deterministic / BQ_DETERMINISTIC), its C ABI, and
the ISA of every kernel its dispatchers launch where the default mode adds with float atomics (_ext.DET_ROUTES): none of them may
hold a float atomic add -- the property that makes a step bitwise reproducible, read from the compiler's output."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")
FLOAT_ATOMIC = re.compile(r"\b(global_atomic_add_f32|buffer_atomic_add_f32|flat_atomic_add_f32|global_atomic_pk_add_\w+|"
                          r"buffer_atomic_pk_add_\w+|flat_atomic_pk_add_\w+)\b")


def _flag_in_fresh_process(env_value):
    env = dict(os.environ)
    env.pop("BQ_DETERMINISTIC", None)
    if env_value is not None:
        env["BQ_DETERMINISTIC"] = env_value
    out = subprocess.run([sys.executable, "-c", "import bridgeqa_amd as b; print(b.is_deterministic())"], cwd=ROOT, env=env,
                         capture_output=True, text=True, check=True).stdout
    return out.strip()


def test_the_mode_is_off_by_default_and_the_environment_variable_sets_it():
    assert _flag_in_fresh_process(None) == "False"
    assert _flag_in_fresh_process("0") == "False"
    assert _flag_in_fresh_process("1") == "True"


def test_set_deterministic_returns_the_previous_value():
    import bridgeqa_amd
    from bridgeqa_amd import fusion_ops
    start = bridgeqa_amd.is_deterministic()
    try:
        assert bridgeqa_amd.set_deterministic(True) == start
        assert bridgeqa_amd.is_deterministic() and fusion_ops.is_deterministic()
        assert bridgeqa_amd.set_deterministic(False) is True
        assert not bridgeqa_amd.is_deterministic()
        assert fusion_ops.set_deterministic(False) is False
    finally:
        bridgeqa_amd.set_deterministic(start)
    assert callable(bridgeqa_amd.manual_seed)


def test_the_new_entry_points_are_declared_and_exported():
    import ctypes
    from bridgeqa_amd import _ext
    hdr = open(os.path.join(ROOT, "include", "bqhip_fusion.h")).read()
    assert re.search(r"#define BQ_GEMM_DET 16\b", hdr) and _ext.GEMM_DET == 16
    lib = ctypes.CDLL(_ext.library_path())
    for s in ("bq_drop_add_ln_bwd_det", "bq_drop_add_ln_bwd_det_slab_floats", "bq_colsum_grouped_det_bf16",
              "bq_colsum_grouped_det_floats", "bq_gemm_splitk_fold_det"):
        assert re.search(r"BQ_API\s+\w+\s+%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
    for site in _ext.DET_ROUTES.values():
        assert hasattr(lib, site["entry"]), site
    # the LayerNorm slab: (workgroups <= 384) x groups x 2H floats
    assert lib.bq_drop_add_ln_bwd_det_slab_floats(16400, 768, 1) == 384 * 2 * 768
    assert lib.bq_drop_add_ln_bwd_det_slab_floats(640, 768, 2) == 80 * 2 * 2 * 768


_ASM = {}


def _asm(src):
    import isa_waits
    if src not in _ASM:
        _ASM[src] = isa_waits.scan(os.path.join(ROOT, "bridgeqa_amd", "csrc", src))
    return _ASM[src]


def _instances(src, name):
    """the mangled kernels of `src` whose identifier is exactly `name` (any template arguments)"""
    pat = re.compile(r"^_ZN2bq%d%s[EI]" % (len(name), name))
    return {k: v for k, v in _asm(src).items() if pat.match(k)}


def test_the_registry_covers_every_atomic_site_of_the_training_path():
    from bridgeqa_amd import _ext
    assert _ext.DET_ROUTES
    for site in ("ln_bwd", "colsum_grouped", "gemm_splitk_f32", "gemm_epilogue_colsum"):
        assert site in _ext.DET_ROUTES and _ext.DET_ROUTES[site]["kernels"], site


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_kernels_of_the_deterministic_mode_hold_no_float_atomic():
    from bridgeqa_amd import _ext
    seen = 0
    for site, route in sorted(_ext.DET_ROUTES.items()):
        for name in route["kernels"]:
            ks = _instances(route["src"], name)
            assert ks, (site, name)
            for k, lines in ks.items():
                hits = [x.strip() for x in lines if FLOAT_ATOMIC.search(x)]
                assert not hits, (site, k, hits[:3])
                seen += 1
    assert seen >= 15, seen
    # the check can see an atomic: the default forms of the same sites hold them
    assert any(FLOAT_ATOMIC.search(x) for k, v in _instances("ln.hip", "drop_add_ln_bwd_kernel").items() for x in v)
    assert any(FLOAT_ATOMIC.search(x) for k, v in _instances("gemm.hip", "colsum_grouped_kernel").items() for x in v)


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_the_deterministic_gemm_keeps_its_tile_loop_free_of_compiler_fences():
    """the ISA guard of tests/test_isa_waits_cpu.py on gemm64_kernel_det: no compiler vmcnt wait in front of a tile-loop LDS read"""
    import isa_waits
    ks = _instances("gemm.hip", "gemm64_kernel_det")
    assert len(ks) >= 7
    for name, lines in ks.items():
        assert isa_waits.lds_dmas(lines), name
        mf = [i for i, x in enumerate(lines) if "v_mfma" in x]
        bad = [h for h in isa_waits.compiler_waits(lines[:mf[-1]]) if h[1].startswith("ds_read")]
        assert not bad, (name, bad)
        assert not isa_waits.lds_read_hazards(lines), name
