"""Kernel-argument preload (csrc/Makefile: -amdgpu-kernarg-preload-count) as the generated code shows it - compiled for gfx950 with the
Makefile's ML_FLAGS, device side only, no GPU needed; walked with tests/diag/preload_waits.py:

    ml_spmv_pcg_kernel            14 SGPRs preloaded (five pointers, four integers); from the real entry - behind the compatibility
                                  prologue - NO full wait in front of the first operand load: the fetch of the struct's fields runs
                                  beside the first round trip
    `const LmSlot*` twins         the slot table's pointer preloaded
    a struct by value in front    nothing preloaded: PcgArgs (ml_init / ml_cg_comp), LmSlot and HostSlot twins come out as they were"""
import importlib.util
import os
import subprocess

import pytest

from test_pcg_prologue_isa import CSRC, HIPCC, _ml_flags

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc (cross-compiles for gfx950 without a GPU)")


def _preload_module():
    spec = importlib.util.spec_from_file_location("preload_waits", os.path.join(HERE, "diag", "preload_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    assert any(f.startswith("-amdgpu-kernarg-preload-count=") for f in _ml_flags()), _ml_flags()
    out = tmp_path_factory.mktemp("isa") / "pgo_ml_kernels.s"
    cmd = [HIPCC] + _ml_flags() + ["--cuda-device-only", "-S", os.path.join(CSRC, "pgo_ml_kernels.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = out.read_text().splitlines()
    pl = _preload_module()
    return [pl.report(lines, name, at) for name, at in pl._pw.kernels(lines, r"^_Z.*_kernel")]


def _named(reports, needle):
    got = [r for r in reports if needle in r["kernel"]]
    assert got, needle
    return got


def test_ml_spmv_first_loads_need_no_wait(reports):
    (r,) = _named(reports, "ml_spmv_pcg_kernel")
    print(r)
    assert r["preload_sgprs"] == 14, r
    assert r["first_operand_load_line"] is not None and r["waits"] == 0, r


def test_slot_table_pointer_is_preloaded(reports):
    twins = _named(reports, "PKNS_6LmSlotE")             # `const LmSlot*` twins: the pointer is their first parameter
    assert len(twins) > 9, len(twins)
    for r in twins:
        assert r["preload_sgprs"] >= 2, r


def test_struct_by_value_kernels_are_unchanged(reports):
    by_value = _named(reports, "ml_init_pcg_kernel") + _named(reports, "ml_cg_comp_pcg_kernel") \
        + [r for r in reports if "_lm_kernelI" in r["kernel"] and ("NS_6LmSlotEE" in r["kernel"] or "NS_8HostSlotEE" in r["kernel"])
           and "PKNS_" not in r["kernel"]]
    assert len(by_value) > 9, len(by_value)
    for r in by_value:
        assert r["preload_sgprs"] == 0, r
