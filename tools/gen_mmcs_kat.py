#!/usr/bin/env python3
"""Write tests/golden/mmcs_kat.json from the model of the mixed-height matrix commitments (tests/mmcs_model.py: the C oracle's
sponge and Merkle level): three shapes with their matrices, tree, root, one opening and its tampered roots.

    python tools/gen_mmcs_kat.py            # rewrite the file
    python tools/gen_mmcs_kat.py --check    # exit 1 if the committed file is stale
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "mmcs_kat.json")


def text():
    import mmcs_model as MM
    return json.dumps(MM.golden(), indent=1) + "\n"


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
