#!/usr/bin/env python3
"""Write tests/golden/perm_inverse_kat.json from the big-integer model of the inverse permutation
(tests/perm_inverse_model.py): D, M^-1, fifth roots of edge values, preimages of three states and the round ranges of one
trace.

    python tools/gen_perm_inverse_kat.py            # rewrite the file
    python tools/gen_perm_inverse_kat.py --check    # exit 1 if the committed file is stale
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "perm_inverse_kat.json")


def text():
    import perm_inverse_model as M
    return json.dumps(M.golden(), indent=1) + "\n"


def main():
    if "--check" in sys.argv:
        with open(OUT) as f:
            stale = f.read() != text()
        print("stale" if stale else "current")
        sys.exit(1 if stale else 0)
    with open(OUT, "w") as f:
        f.write(text())
    print("wrote", OUT)


if __name__ == "__main__":
    main()
