"""Rewrites the fixtures tests/golden/refpin_<case>.npy from the reference binary oracle/_ref/ref_driver.

    python tools/record_reference_pins.py

Needs the binary (oracle.build_ref() with a reference tree).  Each fixture holds what tests/reference_cases.compress() keeps of the
driver's output for one case (of the records the case's view selects): every record's length, the short records whole and the tails of
the long ones.
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
    every = R.cases() + R.inplace_cases()   # (the second list: the reference where the oracle is NOT it, tests/test_oracle_pins.py)
    for c in every:
        kept = c.view([("", r) for r in c.reference(c.make_input())])   # the kinds play no part in what a fixture holds
        np.save(c.fixture, R.compress([r for _, r in kept]))
        total += os.path.getsize(c.fixture)
    print("%d fixtures, %d bytes" % (len(every), total))


if __name__ == "__main__":
    main()
