"""CPU tier: the library's environment switches have one reader (csrc/tuning.h), they are exactly the ones DESIGN.md's table lists,
and the built library carries no k_mix_dec_mfma instance beyond the nine of its instance list (no timing instance: DBG is 0 in all)."""
import os
import re

import pytest

from tests import decim_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pebblesdr_amd", "csrc")
MFMA = re.compile(rb"_ZN2pgL14k_mix_dec_mfmaILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E")


def _sources(base):
    for dp, _, files in os.walk(base):
        for f in sorted(files):
            if f.endswith((".h", ".hpp", ".hip", ".cpp", ".inc")):
                yield os.path.join(dp, f)


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    return g.build()


def test_one_file_reads_the_environment():
    readers = [p for base in (CSRC, os.path.join(ROOT, "include")) for p in _sources(base) if "getenv" in open(p).read()]
    assert readers == [os.path.join(CSRC, "tuning.h")], readers


def test_switches_read_are_the_design_table():
    read = set(re.findall(r'getenv\("(PEBBLEGPU_[A-Z0-9_]+)"\)', open(os.path.join(CSRC, "tuning.h")).read()))
    table = set(re.findall(r"^\| `(PEBBLEGPU_[A-Z0-9_]+)` \|", open(os.path.join(ROOT, "DESIGN.md")).read(), flags=re.M))
    assert read == table, (sorted(read - table), sorted(table - read))
    assert len(read) == 29
    assert not {"PEBBLEGPU_BANK_DBG", "PEBBLEGPU_FUSE_DBG"} & read


def test_only_the_bank_variants_are_built(lib_path):
    want = {inst + (0, minw) for inst, minw in decim_cases.bank_instances().items()}
    assert len(want) == 9
    built = {tuple(int(v) for v in m) for m in MFMA.findall(open(lib_path, "rb").read())}
    assert built == want, (sorted(built - want), sorted(want - built))
