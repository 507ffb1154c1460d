"""Index of the reference tree that tests/test_citations.py checks citations against, so the test needs no reference
checkout: per source file name its line count, and per anchor (file, function name) the lines that name the function.
Numbers and names only; no reference text is stored.

usage: python tools/make_reference_index.py <reference checkout>   (writes tests/golden/reference_index.json)"""
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))


def lines_of(path):
    """Lines as editors number them (split on LF only: the reference's GBK comments hold bytes str.splitlines
    would also break on)."""
    with open(path, "rb") as fh:
        data = fh.read()
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [ln.decode("latin-1") for ln in lines]


def main(ref):
    from test_citations import ANCHORS

    nlines, text = {}, {}
    for dp, _, fn in os.walk(ref):
        if "/.git" in dp:
            continue
        for f in fn:
            if re.search(r"\.(frag|vert|h|cpp|hpp|c)$", f):
                ls = lines_of(os.path.join(dp, f))
                nlines[f] = max(nlines.get(f, 0), len(ls))
                text.setdefault(f, []).append(ls)
    anchors = {}
    for name, _, word in ANCHORS:
        hits = sorted({i + 1 for ls in text.get(name, []) for i, ln in enumerate(ls) if word in ln})
        anchors.setdefault(name, {})[word] = hits
    with open(os.path.join(REPO, "tests", "golden", "reference_index.json"), "w") as f:
        json.dump({"lines": dict(sorted(nlines.items())), "anchors": anchors}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
