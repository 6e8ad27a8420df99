#!/usr/bin/env python3
"""Record tests/golden/eval_args_golden.json: (return code, mke_last_error text) of every argument vector of
tests/eval_args_cases.py — run on a checkout of the commit BEFORE the evaluator's operand checks became one helper, so that
tests/test_eval_args_abi.py can hold every later commit to the same codes, texts, winners and n == 0 returns.  No GPU needed:
every vector is refused before any HIP call.

    python tests/golden/record_eval_args.py --root <checkout of the parent commit, built> [--out FILE]

--root is the tree whose `multike_amd` package is imported (default: the tree this script lies in); the vectors are always
the ones of the tree this script lies in."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import eval_args_cases as ea  # noqa: E402


def record():
    out = {}
    for entry in ea.ENTRY:
        for vid, over in ea.vectors(entry):
            rc, text = ea.run(entry, over)
            # a vector with rows that passes every check would launch on dummy addresses: the table must hold none
            assert rc < 0 or (rc == 0 and over is not None and not ea.has_rows(entry, over)) or entry.endswith("_temp_bytes"), (entry, vid, rc)
            out[f"{entry}/{vid}"] = [rc, text]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)))
    ap.add_argument("--out", default=os.path.join(HERE, "eval_args_golden.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import multike_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(multike_amd.__file__))) == os.path.abspath(a.root), multike_amd.__file__
    rec = record()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out} ({len(rec)} vectors, {os.path.getsize(a.out)} bytes) from {a.root}")


if __name__ == "__main__":
    main()
