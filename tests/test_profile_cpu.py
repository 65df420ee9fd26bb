"""--fs-no-graph with the profile built on the device (sina_hip_align_profiles): what can be checked without a GPU --
the ABI surface, the refusal of a null context, and that the host's option routing is what it was."""
import ctypes as C
import os
import re

from sina_amd import capi, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_profile_symbols_are_exported_and_declared():
    L = capi.load()
    for s in ("sina_hip_align_profiles", "sina_hip_debug_family_profile"):
        assert s in capi.ABI_SYMBOLS
        assert hasattr(L, s), s
    hdr = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+sina_hip_align_profiles\s*\(", code)
    assert re.search(r"\bint\s+sina_hip_debug_family_profile\s*\(", code)
    # the header cites what the entry point restates, like the other entries
    doc = hdr[:hdr.index("int sina_hip_align_profiles")]
    doc = doc[doc.rindex("/*"):]
    assert "src/align.cpp:428-433" in doc and "src/pseq.cpp" in doc and "src/pseq.h:65-113" in doc
    assert L.sina_hip_abi_version() == 5     # (a function was added, no structure changed)


def test_align_profiles_refuses_a_null_context_with_a_message():
    L = capi.load()
    p = capi.AlignParams()
    L.sina_hip_align_params_default(C.byref(p))
    assert L.sina_hip_align_profiles(None, None, None, 0, None, None, C.byref(p), None, None) != 0
    msg = L.sina_hip_last_error()
    assert b"align_profiles" in msg and b"null" in msg
    n = C.c_uint32()
    assert L.sina_hip_debug_family_profile(None, None, 1, -2.0, 1.0, 5.0, 2.0, C.byref(n), None, None, None, 0) != 0
    assert b"debug_family_profile" in L.sina_hip_last_error()
    # the entry point it shares its launch loop with still names itself
    assert L.sina_hip_align_families(None, None, None, 0, None, None, C.byref(p), None, None) != 0
    assert b"align_families" in L.sina_hip_last_error()


def test_host_option_routing_is_unchanged():
    H = pipeline.load_host()
    H.sina_host_reset_options()
    try:
        for v in (b"1", b"0"):
            assert H.sina_host_set_option(b"aligner", b"device-graph", v) == 0
            assert H.sina_host_set_option(b"aligner", b"fs-no-graph", v) == 0
        assert H.sina_host_set_option(b"aligner", b"device-graph", b"1") == 0
        assert H.sina_host_set_option(b"aligner", b"fs-no-graph", b"1") == 0     # both at once: still the host build ...
        assert H.sina_host_set_option(b"aligner", b"device-profile", b"1") == 0  # ... until this asks for the device route
        assert H.sina_host_set_option(b"aligner", b"use-subst-matrix", b"1") != 0
        assert H.sina_host_set_option(b"aligner", b"no-such-option", b"1") != 0
    finally:
        H.sina_host_reset_options()
