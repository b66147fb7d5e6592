#!/usr/bin/env python3
"""Records the accuracy of technique 8's slab classification (vrhip_preint_slab) against the extended-precision
evaluation of tests/test_preint_ref.py: the largest absolute error per channel and table size, written to
profiles/r4/preint_accuracy.json.  tests/test_preint_ref.py allows 4 x these values, at most 1e-6.  No GPU."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import test_preint_ref as T   # noqa: E402
from volumerenderercl_amd import _srchash   # noqa: E402


def main():
    out = {"what": "max |vrhip_preint_slab - extended-precision evaluation| per channel (r, g, b, a), random RGBA8 "
                   "tables, 10^4 random intervals per table size, a fifth of them a few ulps long",
           "library_source_hash": _srchash.source_hash(), "max_abs_error": {}, "intervals": {}, "shorter_than_2^-20_texel": {}}
    for n in T.SIZES:
        err, short, count = T.measure_errors(n)
        out["max_abs_error"][str(n)] = err
        out["intervals"][str(n)] = count
        out["shorter_than_2^-20_texel"][str(n)] = short
        print(n, err, count, short)
    with open(T.ACCURACY, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
