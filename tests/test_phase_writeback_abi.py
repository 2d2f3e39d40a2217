"""The interface of the phase write-back interval (include/datum_ocean_hip.h: datum_ocean_set_phase_writeback, datum_ocean_phase_writeback):
declared, exported, bound, argument checks that need no device, and the ABI number it was added under.  The checks that need a handle
(range, DATUM_OCEAN_ESTATE under an open profile) are the one GPU test at the end."""

import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "datum_ocean_hip.h")
MODULE = os.path.join(ROOT, "datum_amd", "csrc", "ocean_capi.hip")

SYMBOLS = ("datum_ocean_set_phase_writeback", "datum_ocean_phase_writeback")


def _text(path):
    return open(path, encoding="utf-8").read()


def test_header_declares_and_library_exports():
    from datum_amd import capi

    text = _text(HEADER)
    lib = capi.load()
    assert re.search(r"int\s+datum_ocean_set_phase_writeback\s*\(\s*datum_ocean_t\s+ctx\s*,\s*int\s+every\s*\)\s*;", text)
    assert re.search(r"int\s+datum_ocean_phase_writeback\s*\(\s*datum_ocean_t\s+ctx\s*,\s*int\s*\*\s*every\s*\)\s*;", text)
    for name in SYMBOLS:
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert capi.SYMBOLS["datum_ocean_set_phase_writeback"] == (capi.I, [capi.P, capi.I])
    assert capi.SYMBOLS["datum_ocean_phase_writeback"] == (capi.I, [capi.P, ctypes.POINTER(capi.I)])


def test_abi_number_is_still_nine_and_the_header_says_how_to_probe():
    from datum_amd import capi

    assert capi.ABI_VERSION == capi.header_abi_version() == capi.load().datum_ocean_abi_version() == 9
    text = _text(HEADER)
    history = text[text.index("Version of THIS header's contract"):text.index("#define DATUM_OCEAN_ABI_VERSION")]
    for name in SYMBOLS:
        assert name in history, name
    assert "detects them by symbol" in history
    # what a caller may assume about the phase is stated next to the declaration
    assert "WHAT A CALLER MAY ASSUME" in text and "the value they see is the one the every-step path would hold" in text.lower()


def test_binding_has_the_two_methods():
    from datum_amd import capi

    for name in ("set_phase_writeback", "phase_writeback"):
        assert callable(getattr(capi.Ocean, name)), name


def test_argument_errors_without_gpu():
    from datum_amd import capi

    lib = capi.load()
    every = capi.I(-7)
    assert lib.datum_ocean_set_phase_writeback(None, 4) == capi.EINVAL
    assert b"datum_ocean_set_phase_writeback" in lib.datum_ocean_last_error(None)
    assert lib.datum_ocean_phase_writeback(None, ctypes.byref(every)) == capi.EINVAL
    assert b"datum_ocean_phase_writeback" in lib.datum_ocean_last_error(None)
    assert every.value == -7


def test_setters_of_the_plan_are_refused_under_an_open_profile_in_the_source():
    # every setter that feeds plan_step answers DATUM_OCEAN_ESTATE while a profile is open -- this one and the spectrum format among them
    text = _text(MODULE)
    for name in ("datum_ocean_set_phase_writeback", "datum_ocean_set_spectrum_format", "datum_ocean_set_cascade_group", "datum_ocean_set_map_store_policy"):
        start = text.index("int " + name + "(")
        body = text[start:text.index("\n}\n", start)]
        assert re.search(r"if \(ctx->profiling\)\s*\n\s*return fail\(ctx, DATUM_OCEAN_ESTATE", body), name


def test_default_interval_is_a_constant_of_the_plan():
    from datum_amd import capi

    text = _text(MODULE)
    m = re.search(r"constexpr int PHASE_WRITEBACK_EVERY = (\w+);", text)
    assert m
    plan = text[text.index("StepPlan plan_step("):text.index("template<int N>\n  StepKernels step_kernels()")]
    assert "PHASE_WRITEBACK_EVERY" in plan
    assert "#define PHASE_WRITEBACK" not in text and "getenv" not in text
    k = m.group(1)
    k = 8 if k == "MAX_PENDING" else int(k)
    assert 1 <= k <= 8
    assert capi.ABI_VERSION == 9


@pytest.mark.gpu
def test_range_getter_and_estate_under_an_open_profile():
    import numpy as np

    from datum_amd import capi

    with capi.Ocean(64, 1) as oc:
        default = oc.phase_writeback()
        assert 1 <= default <= 8
        for bad in (-1, 9, 100):
            with pytest.raises(capi.OceanError) as e:
                oc.set_phase_writeback(bad)
            assert e.value.code == capi.EINVAL
            assert oc.phase_writeback() == default
        for k in range(1, 9):
            oc.set_phase_writeback(k)
            assert oc.phase_writeback() == k
        oc.set_phase_writeback(0)
        assert oc.phase_writeback() == default
        with pytest.raises(capi.OceanError) as e:
            oc._check(oc.lib.datum_ocean_phase_writeback(oc.h, None))
        assert e.value.code == capi.EINVAL
        oc.upload_state(0, np.zeros((64, 64, 2), np.float32))
        oc.profile_begin(4)
        with pytest.raises(capi.OceanError) as e:
            oc.set_phase_writeback(2)
        assert e.value.code == capi.ESTATE
        with pytest.raises(capi.OceanError) as e:
            oc.set_spectrum_format("fp16")
        assert e.value.code == capi.ESTATE
        assert oc.phase_writeback() == default
        oc.profile_end()
        oc.set_phase_writeback(2)
        assert oc.phase_writeback() == 2
