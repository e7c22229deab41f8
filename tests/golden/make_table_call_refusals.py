"""Generates tests/golden/table_call_refusals.json: the complete musica_last_error() string of every refusal that
tests/test_gpu_table_call_refusals.py provokes from musica_sim_profiles / _levels / _gradients / _order / _reach, as the library built
from the commit named in the file words them. It needs a GPU. The strings are a pin of the ABI's refusals against rewording and
reordering by later work on the host code: record them from a commit BEFORE such work, never from the tree under test.

Run from the repo root:  python tests/golden/make_table_call_refusals.py <commit the library was built from>
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_table_call_refusals as T  # noqa: E402


def main():
    out = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
    json.dump({"recorded_from": sys.argv[1], "refusals": T.refusals()}, open(out, "w"), indent=1)
    print("%d refusals -> %s" % (len(json.load(open(out))["refusals"]), out))


if __name__ == "__main__":
    main()
