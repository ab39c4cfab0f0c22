#!/usr/bin/env python3
"""Write tests/golden/matrix_kat.json from the model of the matrix commitments (tests/matrix_model.py: a transpose over the
C oracle's sponge and Merkle tree): three small matrices with digests, tree, root and one opening each.

    python tools/gen_matrix_kat.py            # rewrite the file
    python tools/gen_matrix_kat.py --check    # exit 1 if the committed file is stale
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "matrix_kat.json")


def text():
    import matrix_model as M
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
