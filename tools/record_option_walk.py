#!/usr/bin/env python3
"""Record what every option, counter and timed kernel name of the C ABI does: tests/golden/option_walk.json.

    python3 tools/record_option_walk.py [out.json]

The walk is tests/option_walk.py (its docstring says what a cell is).  It is made twice in one process and the two must agree: a cell
that is not repeatable has no place in the recording.  One line per cell.  The digests are those of the MI355X; codes, texts and counts
do not depend on the card.  Run it on the commit whose behaviour is to be kept.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import option_walk as walk  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "option_walk.json")
    cells = walk.walk()
    handles = walk.handles_made
    again = walk.walk()
    unstable = [k for k in cells if cells[k] != again[k]]
    assert not unstable, f"{len(unstable)} cells differ between two walks, first: {[(k, cells[k], again[k]) for k in unstable[:3]]}"
    lines = ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}" for k, v in cells.items())
    doc = ('{"key":"section|handle kind|name|position:value","shapes":' + json.dumps(walk.SHAPES, separators=(",", ":"))
           + ',\n"cells":{\n' + lines + "\n}}\n")
    json.loads(doc)
    with open(out, "w") as f:
        f.write(doc)
    print(f"{len(cells)} cells, {sum(v[0] != 0 for v in cells.values())} refused, {handles} handles per walk, {len(doc)} bytes -> {out}")


if __name__ == "__main__":
    main()
