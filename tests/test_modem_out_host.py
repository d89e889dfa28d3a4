"""CPU tier of the modem hook ring (pebblegpu_receiver_modem_out_*, include/pebblegpu.h): the block layout function for odd row and
super-frame counts, the host twin of the packing kernel against pebblegpu_iq_record_convert, the block struct against its declaration,
the argument refusals that need no device, and that the plain-C host and the C++ feeder compile and link.  tests/test_modem_out_gpu.py
holds the ring itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import modem_out_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    g.build()
    import pebblesdr_amd as P
    return P


@pytest.mark.parametrize("fmt", [MC.F32, MC.S16])
def test_layout_for_odd_rows_and_superframes(P, fmt):
    """rows of any length are padded to 16 bytes, the trailer starts right behind the last row and is padded to 16 bytes itself; every
    combination of 1..9 and 16 rows, odd and even row lengths, and 1, 2, 3, 5, 8 and 17 super-frames"""
    seen = set()
    for rows in list(range(1, 10)) + [16]:
        for k in (1, 2, 3, 5, 8, 17):
            for n in [k * m for m in (1, 2, 3, 5, 7, 64, 2048, 2049)]:
                pitch, off, nbytes = P.modem_out_layout(fmt, rows, n, k)
                assert (pitch, off, nbytes) == MC.layout_ref(fmt, rows, n, k)
                assert pitch % 16 == 0 and pitch >= n * MC.BYTES[fmt] and pitch - n * MC.BYTES[fmt] < 16
                assert off == rows * pitch and nbytes % 16 == 0 and 0 <= nbytes - rows * k < 16
                seen.add((n * MC.BYTES[fmt] % 16 != 0, rows * k % 16 != 0))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}   # padded and unpadded rows, padded and unpadded trailers
    assert P.modem_out_layout(fmt, 3, 0, 0) == (0, 0, 0)


def test_convert_twin_against_the_record_twin(P):
    """S16 is pebblegpu_iq_record_convert, value for value (truncation, saturation to +-32767, NaN -> 0); F32 hands the floats on verbatim,
    NaN payloads and signed zeros included"""
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.uniform(-1.2, 1.2, 4000), [0.0, -0.0, 1.0, -1.0, 0.99999, 1.00001, 3.0, -3.0, np.inf, -np.inf, np.nan, 1e-9, -1e-9, 0.5 / 32767]])
    iq = np.stack([v, v[::-1]], axis=1).astype(np.float32)
    s16 = P.modem_out_convert(MC.S16, iq)
    assert s16.dtype == np.int16 and np.array_equal(s16, P.iq_record_convert(iq))
    assert s16.max() == 32767 and s16.min() == -32767 and (s16 == 0).any()
    f32 = P.modem_out_convert(MC.F32, iq)
    assert f32.dtype == np.float32 and f32.tobytes() == iq.tobytes()
    assert P.modem_out_convert(MC.F32, np.zeros((0, 2), dtype=np.float32)).shape == (0, 2)


def test_refusals_that_need_no_device(P):
    L = P.load_library()

    def code(rc):
        return rc

    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    x = np.zeros((4, 2), dtype=np.float32)
    out = np.zeros((4, 2), dtype=np.float32)
    xp, op = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert code(L.pebblegpu_modem_out_convert(MC.S16_MONO, xp, 4, op)) == MC.E_INVALID      # left-only PCM is an audio format
    assert code(L.pebblegpu_modem_out_convert(3, xp, 4, op)) == MC.E_INVALID
    assert code(L.pebblegpu_modem_out_convert(-1, xp, 4, op)) == MC.E_INVALID
    assert code(L.pebblegpu_modem_out_convert(MC.F32, None, 4, op)) == MC.E_INVALID
    assert code(L.pebblegpu_modem_out_convert(MC.F32, xp, 4, None)) == MC.E_INVALID
    assert code(L.pebblegpu_modem_out_convert(MC.F32, None, 0, None)) == 0
    assert code(L.pebblegpu_modem_out_layout(MC.S16_MONO, 1, 1, 1, C.byref(a), C.byref(b), C.byref(c))) == MC.E_INVALID
    assert code(L.pebblegpu_modem_out_layout(MC.F32, 1, 1, 1, None, C.byref(b), C.byref(c))) == MC.E_INVALID
    blk = P.ModemBlock()
    blk.struct_size = C.sizeof(P.ModemBlock)
    d = C.c_uint64()
    assert code(L.pebblegpu_receiver_modem_out_open(None, MC.F32, None, 0, 4)) == MC.E_INVALID  # null handles
    assert code(L.pebblegpu_receiver_modem_out_close(None)) == MC.E_INVALID
    assert code(L.pebblegpu_receiver_modem_out_next(None, 0, C.byref(blk))) == MC.E_INVALID
    assert code(L.pebblegpu_receiver_modem_out_release(None, 0)) == MC.E_INVALID
    assert code(L.pebblegpu_receiver_modem_out_dropped(None, C.byref(d))) == MC.E_INVALID
    assert b"null" in L.pebblegpu_last_error()


def test_block_struct_matches_its_declaration(P, tmp_path):
    """sizeof and every field's offset, as a C compiler lays pebblegpu_modem_block out, against the binding's ctypes structure; the audio
    block's fields come first, in its order"""
    fields = [f for f, _ in P.ModemBlock._fields_]
    assert fields[:8] == [f for f, _ in P.AudioBlock._fields_]
    assert fields[8:] == ["rate", "n_superframes", "samples_per_superframe", "present"]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pebblegpu.h"', 'int main(void) {', 'printf("%zu\\n", sizeof(pebblegpu_modem_block));']
    lines += ['printf("%%zu\\n", offsetof(pebblegpu_modem_block, %s));' % f for f in fields]
    lines += ['return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(P.ModemBlock)] + [getattr(P.ModemBlock, f).offset for f in fields]


def test_the_c_host_and_the_feeder_compile(P, tmp_path):
    lib = os.path.join(ROOT, "pebblesdr_amd")
    inc = "-I" + os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", inc, os.path.join(ROOT, "examples", "modem_out_host.c"), "-L" + lib, "-lpebblegpu",
                           "-Wl,-rpath," + lib, "-lm", "-lpthread", "-o", str(tmp_path / "modem_out_host")])
    src = tmp_path / "feeder.cpp"
    src.write_text(MC.FEEDER_CPP)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", inc, str(src), "-L" + lib, "-lpebblegpu", "-Wl,-rpath," + lib, "-o", str(tmp_path / "feeder")])


def test_header_and_documents_state_the_semantics():
    """the header pins the source, the read-only rule, absent pairs and the trailer; DESIGN.md section 7 no longer leaves host decoders without
    a path"""
    hdr = open(os.path.join(ROOT, "include", "pebblegpu.h")).read()
    for phrase in ("receiver.cpp:979-980", "READ-ONLY", "ABSENT PAIRS", "receiver.cpp:962-965", ":968-971", "padded to 16 bytes", "PEBBLEGPU_TAP_MODEM shows"):
        assert phrase in hdr, phrase
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "pebblegpu_receiver_modem_out_open" in design and "k_modem_pack" in design
