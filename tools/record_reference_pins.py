"""Rewrites the fixtures tests/golden/refpin_<case>.npy from the reference binary oracle/_ref/ref_driver.

    python tools/record_reference_pins.py

Needs the binary (oracle.build_ref() with a reference tree).  Each fixture holds what tests/reference_cases.compress() keeps of the
driver's output for one case: every record's length, the short records whole and the tails of the long ones.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import oracle
    from tests import reference_cases as R
    if not oracle.build_ref():
        sys.exit("no reference binary and no reference tree to build it from")
    total = 0
    for c in R.cases():
        np.save(c.fixture, R.compress(c.reference(c.make_input())))
        total += os.path.getsize(c.fixture)
    print("%d fixtures, %d bytes" % (len(R.cases()), total))


if __name__ == "__main__":
    main()
