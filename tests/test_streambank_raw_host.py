"""CPU tier of the stream bank's raw-format input (pebblegpu_streambank_process_raw, the pinned ingest slots, kernel_name): the
header declares the calls, the built library exports them, the binding lists them and StreamBank carries the methods.  No compute
call is made here: without a device the bank refuses to exist."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pebblegpu.h")
NEW = ["pebblegpu_streambank_process_raw", "pebblegpu_streambank_ingest_acquire", "pebblegpu_streambank_ingest_submit",
       "pebblegpu_streambank_process_ingested", "pebblegpu_streambank_kernel_name"]


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    return g.build()


def _header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_raw_calls_and_states_the_alignment():
    code = _header_code()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    m = re.search(r"#define\s+PEBBLEGPU_RAW_ALIGN\s+(\d+)", code)
    assert m and int(m.group(1)) == 32  # covers the widest load of any sample format (four float pairs)
    # the raw call carries format, order, gain and `what`; process_ingested the slot in front of them
    assert re.search(r"pebblegpu_streambank_process_raw\s*\(\s*pebblegpu_streambank \*\w+,\s*int \w+,\s*int \w+,\s*double \w+,\s*const void \*\w+,\s*"
                     r"uint64_t \w+,\s*uint32_t \w+\)", code)
    assert re.search(r"pebblegpu_streambank_process_ingested\s*\(\s*pebblegpu_streambank \*\w+,\s*uint32_t \w+,\s*int \w+,\s*int \w+,\s*double \w+,\s*"
                     r"uint64_t \w+,\s*uint32_t \w+\)", code)
    assert re.search(r"const char \*pebblegpu_streambank_kernel_name\s*\(\s*const pebblegpu_streambank \*\w+,\s*int \w+\)", code)


def test_library_exports_the_raw_calls_for_gfx950_only(lib_path):
    L = ctypes.CDLL(lib_path)
    missing = [f for f in NEW if not hasattr(L, f)]
    assert not missing, missing
    assert L.pebblegpu_abi_version() == 1  # additive: the version stays
    blob = open(lib_path, "rb").read()
    assert set(re.findall(rb"amdgcn-amd-amdhsa--(gfx[0-9a-z]+)", blob)) == {b"gfx950"}
    # the converting instances are in the code object, one per sample format
    for kern in (b"k_fastfir_t128_raw", b"k_big256_cols_raw"):
        assert blob.count(kern) >= 5, kern


def test_binding_lists_the_calls_and_streambank_has_the_methods(lib_path):
    from pebblesdr_amd import binding as B
    for name in NEW:
        assert name in B.SYMBOLS
        assert getattr(B.load_library(), name).argtypes is not None
    for meth in ("process_raw_device", "ingest_acquire", "ingest_submit", "process_ingested", "kernel_name"):
        assert callable(getattr(B.StreamBank, meth)), meth


def test_null_handles_are_refused_not_dereferenced(lib_path):
    from pebblesdr_amd import binding as B
    L = B.load_library()
    p = ctypes.c_void_p()
    assert L.pebblegpu_streambank_process_raw(None, 0, 0, 1.0, None, 0, 3) == -1
    assert L.pebblegpu_streambank_ingest_acquire(None, 0, 16, ctypes.byref(p)) == -1
    assert L.pebblegpu_streambank_ingest_submit(None, 0, 16) == -1
    assert L.pebblegpu_streambank_process_ingested(None, 0, 0, 0, 1.0, 0, 3) == -1
    assert L.pebblegpu_streambank_kernel_name(None, 1) == b""


def test_no_device_is_still_a_loud_failure(lib_path):
    """Without a device creating a bank must fail with PEBBLEGPU_E_NO_DEVICE: the raw route has no CPU path either.  (Where a device
    is visible the bank exists and has run nothing yet: no route to name.)"""
    import pebblesdr_amd as P
    L = P.load_library()
    if L.pebblegpu_device_count() > 0:
        sb = P.StreamBank(2.0e6, 4)
        assert sb.kernel_name(1) == "" and sb.kernel_name(2) == ""
        sb.close()
        return
    with pytest.raises(P.PebbleGpuError) as e:
        P.StreamBank(2.0e6, 4)
    assert e.value.code == -2
